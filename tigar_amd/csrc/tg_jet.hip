// SECOND-DERIVATIVE point forms on mapped tensor-product patches: what a user of the reference writes in terms of
// spline.parametricGrad(x) and its derivative -- a Kirchhoff-Love shell energy (demos/kl-shell-svk) -- needs the first and
// second PARAMETRIC derivatives of the unknown and of the geometry at the quadrature points, and forms whose point data
// act on them.
//
// The JET of a function at a point: value | first derivatives | second derivatives in the order 00, 01, 11 (k <= m);
// nJ = 3 components for d = 1, 6 for d = 2.  Derivatives refer to the patch's parametric (knot) coordinates xi, NOT to the
// reference element [0,1]^d the tables l | dl | d2l live on: with h_k the element's size in direction k
//     jet_xi = S jet_ref,  S = diag(1, 1/h_k, 1/(h_k h_m)).
// RATIONAL functions psi = phi / W_h: with omega = 1/W, d_k omega = -W_k / W^2, d_km omega = -W_km / W^2 + 2 W_k W_m / W^3
//     psi = omega phi,   d_k psi = omega d_k phi + d_k omega phi,
//     d_km psi = omega d_km phi + d_k omega d_m phi + d_m omega d_k phi + d_km omega phi
// i.e. jet(psi) = L jet(phi), L lower triangular, built from the jet of W_h.  Q = S L_ref (L = I without `rational`) is the
// one matrix per point everything here uses: jet_xi(u) = Q jet_ref(u_h); the geometry is always x = N / W, so
// jet_xi(x_c) = Q_rational jet_ref(N_c).  Point data T (nJ x nJ per block, row = test, column = trial) and s (nJ per field)
// given against xi-jets of the functions of the space come to the reference element as
//     T' = wdet Q^T T Q        s' = wdet Q^T s          (wdet: the weight of tg_quad_points)
// and the element kernels need one variant, no control functions and no element sizes:
//     A_e[a][b] = sum_q sum_ab J^a_ref phi_a T'^ab_q J^b_ref phi_b        out[a] = sum_q sum_a s'^a_q J^a_ref phi_a.
//
// Scope: d = 1, 2, nsd >= d, the scalar Q_p space (nF fields share it, dofs field after field).  Points and point arrays are
// numbered as tg_quad_points, component-major: component alpha of field i at (i nJ + alpha) npts + q.
//
// k_jet_points: a workgroup of 256 threads takes max(1, 256 / nq^d) elements; the nodal values of the nsd + 1 control
// functions (and of u) go to LDS, then one thread per point forms the reference jets directly (O((p+1)^d) per field: d <= 2)
// and ends in one of four ways.  k_jet_matrix / k_jet_load: one workgroup per element, the tables and the element's point
// data in LDS, one thread per pair (a, b) / per node a; elements of one launch share no node (the colours of
// k_assemble_mapped, in the same order) and add without atomics: the same inputs give the same bits.
// Every loop over threads strides by the block size: a one-thread host build is valid (tools/jet_host_sweep.cpp).
#include "tg_common.h"
#include "tg_point_shared.h"
#include <cmath>
#include <vector>

#define TG_JET_POINTS_U 0        // jet_xi(u)
#define TG_JET_POINTS_GEOM 1     // jet_xi(x_c), c < nsd
#define TG_JET_POINTS_T 2        // T' = wdet Q^T T Q, nblk blocks
#define TG_JET_POINTS_S 3        // s' = wdet Q^T s, nblk fields

struct tg_jet_args {
  int p, nsd, nq;
  int nel[3], n[3];            // elements / nodes per direction (1 beyond d)
  const double *f[5];          // nodal fields: 0..2 homogeneous coordinates (the first nsd), 3 the weight function, 4 u (or null)
  int nc;                      // how many of them there are
  const double *tab;           // l[a][q] | dl[a][q] | w[q] | d2l[a][q]
  const double *verts[2];      // element vertices per direction (device)
  int epg;                     // k_jet_points: elements per workgroup
  int64_t nelem, npts, nnodes;
  int nblk;                    // blocks of T / fields of s
  const double *in;            // T_q / s_q (k_jet_points); the transformed data (k_jet_matrix, k_jet_load)
  double *out;
  const int64_t *rowptr;       // k_jet_matrix: the element-coupling pattern
  double *val;
  int efirst[3], ncol[3];      // k_jet_matrix, k_jet_load: the elements efirst[k] + 2 i, i < ncol[k]
};

// reference jet of the tensor-product Lagrange function (a0, a1) at the point (q0, q1): constant indices, registers
template <int D>
__device__ __forceinline__ void tg_jet_basis(const double *tl, const double *tdl, const double *td2, int nq, int a0, int a1, int q0,
                                             int q1, double *B) {
  const double l0 = tl[a0 * nq + q0], d0 = tdl[a0 * nq + q0], e0 = td2[a0 * nq + q0];
  if constexpr (D == 1) {
    B[0] = l0, B[1] = d0, B[2] = e0;
  } else {
    const double l1 = tl[a1 * nq + q1], d1 = tdl[a1 * nq + q1], e1 = td2[a1 * nq + q1];
    B[0] = l0 * l1, B[1] = d0 * l1, B[2] = l0 * d1, B[3] = e0 * l1, B[4] = d0 * d1, B[5] = l0 * e1;
  }
}

// L of jet(phi / W) = L jet(phi) from the jet of W (any coordinates); every entry is written, the zeros as literals
template <int D>
__device__ __forceinline__ void tg_jet_quotient(const double *Wj, double (*L)[D == 1 ? 3 : 6]) {
  constexpr int NJ = D == 1 ? 3 : 6;
#pragma unroll
  for (int a = 0; a < NJ; a++)
#pragma unroll
    for (int b = 0; b < NJ; b++) L[a][b] = 0.0;
  const double om = 1.0 / Wj[0], om2 = om * om, om3 = om2 * om;
#pragma unroll
  for (int a = 0; a < NJ; a++) L[a][a] = om;
  if constexpr (D == 1) {
    const double o0 = -Wj[1] * om2;
    L[1][0] = o0;
    L[2][0] = -Wj[2] * om2 + 2.0 * Wj[1] * Wj[1] * om3;
    L[2][1] = 2.0 * o0;
  } else {
    const double o0 = -Wj[1] * om2, o1 = -Wj[2] * om2;
    L[1][0] = o0;
    L[2][0] = o1;
    L[3][0] = -Wj[3] * om2 + 2.0 * Wj[1] * Wj[1] * om3;
    L[4][0] = -Wj[4] * om2 + 2.0 * Wj[1] * Wj[2] * om3;
    L[5][0] = -Wj[5] * om2 + 2.0 * Wj[2] * Wj[2] * om3;
    L[3][1] = 2.0 * o0;
    L[4][1] = o1;
    L[4][2] = o0;
    L[5][2] = 2.0 * o1;
  }
}

template <int D, int MODE, bool RAT>
__global__ void __launch_bounds__(256) k_jet_points(tg_jet_args P) {
  constexpr int NJ = D == 1 ? 3 : 6;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int p1 = P.p + 1, nq = P.nq, nsd = P.nsd, epg = P.epg;
  const int nloc = D == 1 ? p1 : p1 * p1, nqt = D == 1 ? nq : nq * nq;
  const int szE = P.nc * nloc;
  double *tl = reinterpret_cast<double *>(smem);   // l[a][q]
  double *tdl = tl + p1 * nq;                      // dl[a][q]
  double *tw = tdl + p1 * nq;                      // w[q]
  double *td2 = tw + nq;                           // d2l[a][q]
  double *buf = td2 + p1 * nq;                     // [element][field][local node]
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t g0 = (int64_t)blockIdx.x * epg;
  for (int s = tid; s < 3 * p1 * nq + nq; s += nt) tl[s] = P.tab[s];
  for (int i = tid; i < epg * nloc; i += nt) {
    const int es = i / nloc, a = i - es * nloc;
    const int64_t e = g0 + es;
    if (e >= P.nelem) continue;
    const int el0 = (int)(e % P.nel[0]), el1 = (int)(e / P.nel[0]);
    const int64_t node = (int64_t)(el0 * P.p + a % p1) + (int64_t)P.n[0] * (el1 * P.p + a / p1);
#pragma unroll
    for (int c = 0; c < 5; c++)
      if (tg_pt_has(c, nsd, P.f)) buf[(size_t)es * szE + tg_pt_ci(c, nsd) * nloc + a] = P.f[c][node];
  }
  __syncthreads();
  for (int i = tid; i < epg * nqt; i += nt) {
    const int es = i / nqt, q = i - es * nqt;
    const int64_t e = g0 + es;
    if (e >= P.nelem) continue;
    const int el0 = (int)(e % P.nel[0]), el1 = (int)(e / P.nel[0]);
    const int q0 = q % nq, q1 = q / nq;
    // reference jets of the nodal fields
    double J[5][NJ];
#pragma unroll
    for (int c = 0; c < 5; c++)
#pragma unroll
      for (int al = 0; al < NJ; al++) J[c][al] = 0.0;
    for (int a = 0; a < nloc; a++) {
      double B[NJ];
      tg_jet_basis<D>(tl, tdl, td2, nq, a % p1, a / p1, q0, q1, B);
#pragma unroll
      for (int c = 0; c < 5; c++) {
        if (!tg_pt_has(c, nsd, P.f)) continue;
        const double v = buf[(size_t)es * szE + tg_pt_ci(c, nsd) * nloc + a];
#pragma unroll
        for (int al = 0; al < NJ; al++) J[c][al] = fma(B[al], v, J[c][al]);
      }
    }
    // S, L of the quotient by W_h in reference coordinates, Q = S L
    double S[NJ];
    {
      const double r0 = 1.0 / (P.verts[0][el0 + 1] - P.verts[0][el0]);
      S[0] = 1.0, S[1] = r0;
      if constexpr (D == 1) {
        S[2] = r0 * r0;
      } else {
        const double r1 = 1.0 / (P.verts[1][el1 + 1] - P.verts[1][el1]);
        S[2] = r1, S[3] = r0 * r0, S[4] = r0 * r1, S[5] = r1 * r1;
      }
    }
    [[maybe_unused]] double Qg[NJ][NJ];          // the geometry's (and a rational function's) Q; the plain jet of u needs S alone
    if constexpr (RAT || MODE != TG_JET_POINTS_U) {
      tg_jet_quotient<D>(J[3], Qg);
#pragma unroll
      for (int a = 0; a < NJ; a++)
#pragma unroll
        for (int b = 0; b < NJ; b++)
          if (b <= a) Qg[a][b] *= S[a];
    }
    const int64_t gp = e * nqt + q;   // the point's number in the patch
    if constexpr (MODE == TG_JET_POINTS_U) {
#pragma unroll
      for (int a = 0; a < NJ; a++) {
        double v = 0.0;
        if constexpr (RAT) {
#pragma unroll
          for (int b = 0; b < NJ; b++)
            if (b <= a) v = fma(Qg[a][b], J[4][b], v);
        } else {
          v = S[a] * J[4][a];
        }
        P.out[(int64_t)a * P.npts + gp] = v;
      }
    } else if constexpr (MODE == TG_JET_POINTS_GEOM) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        if (c >= nsd) continue;
#pragma unroll
        for (int a = 0; a < NJ; a++) {
          double v = 0.0;
#pragma unroll
          for (int b = 0; b < NJ; b++)
            if (b <= a) v = fma(Qg[a][b], J[c][b], v);
          P.out[(int64_t)(c * NJ + a) * P.npts + gp] = v;
        }
      }
    } else {
      // wdet as tg_quad_points forms it: DF[c][k] = d(N_c / W)/d xi_k on the reference element, g = DF^T DF
      const double W = J[3][0];
      double DF[3][2] = {{0, 0}, {0, 0}, {0, 0}};
#pragma unroll
      for (int c = 0; c < 3; c++) {
        if (c >= nsd) continue;
#pragma unroll
        for (int k = 0; k < D; k++) DF[c][k] = (J[c][1 + k] * W - J[c][0] * J[3][1 + k]) / (W * W);
      }
      const double g00 = DF[0][0] * DF[0][0] + DF[1][0] * DF[1][0] + DF[2][0] * DF[2][0];
      double det = g00;
      if constexpr (D == 2) {
        const double g01 = DF[0][0] * DF[0][1] + DF[1][0] * DF[1][1] + DF[2][0] * DF[2][1];
        const double g11 = DF[0][1] * DF[0][1] + DF[1][1] * DF[1][1] + DF[2][1] * DF[2][1];
        det = g00 * g11 - g01 * g01;
      }
      const double wdet = tw[q0] * (D == 2 ? tw[q1] : 1.0) * sqrt(fabs(det));
      // Q of the functions of the space: the geometry's, or S alone
      if constexpr (!RAT) {
#pragma unroll
        for (int a = 0; a < NJ; a++)
#pragma unroll
          for (int b = 0; b < NJ; b++) Qg[a][b] = a == b ? S[a] : 0.0;
      }
      if constexpr (MODE == TG_JET_POINTS_T) {
        for (int blk = 0; blk < P.nblk; blk++) {
          const double *Tq = P.in + (int64_t)blk * NJ * NJ * P.npts + gp;
          double *To = P.out + (int64_t)blk * NJ * NJ * P.npts + gp;
          double T[NJ][NJ], X[NJ][NJ];
#pragma unroll
          for (int a = 0; a < NJ; a++)
#pragma unroll
            for (int b = 0; b < NJ; b++) T[a][b] = Tq[(int64_t)(a * NJ + b) * P.npts];
          // X = T Q, then T' = wdet Q^T X (Q lower triangular)
#pragma unroll
          for (int a = 0; a < NJ; a++)
#pragma unroll
            for (int b = 0; b < NJ; b++) {
              double v = 0.0;
#pragma unroll
              for (int g = 0; g < NJ; g++)
                if (g >= b && (RAT || g == b)) v = fma(T[a][g], Qg[g][b], v);
              X[a][b] = v;
            }
#pragma unroll
          for (int a = 0; a < NJ; a++)
#pragma unroll
            for (int b = 0; b < NJ; b++) {
              double v = 0.0;
#pragma unroll
              for (int g = 0; g < NJ; g++)
                if (g >= a && (RAT || g == a)) v = fma(Qg[g][a], X[g][b], v);
              To[(int64_t)(a * NJ + b) * P.npts] = wdet * v;
            }
        }
      } else {
        for (int i = 0; i < P.nblk; i++) {
          const double *sq = P.in + (int64_t)i * NJ * P.npts + gp;
          double *so = P.out + (int64_t)i * NJ * P.npts + gp;
          double s[NJ];
#pragma unroll
          for (int a = 0; a < NJ; a++) s[a] = sq[(int64_t)a * P.npts];
#pragma unroll
          for (int a = 0; a < NJ; a++) {
            double v = 0.0;
#pragma unroll
            for (int g = 0; g < NJ; g++)
              if (g >= a && (RAT || g == a)) v = fma(Qg[g][a], s[g], v);
            so[(int64_t)a * P.npts] = wdet * v;
          }
        }
      }
    }
  }
}

// element of a coloured launch
template <int D>
__device__ __forceinline__ int64_t tg_jet_colour_element(const tg_jet_args &P, int *el) {
  int64_t e = blockIdx.x;
  el[0] = 2 * (int)(e % P.ncol[0]) + P.efirst[0];
  e /= P.ncol[0];
  el[1] = D == 2 ? 2 * (int)e + P.efirst[1] : 0;
  return (int64_t)el[0] + (int64_t)P.nel[0] * el[1];
}

// block (i, j) of the matrix from its nJ^2 transformed values per point (P.in: that block's slice)
template <int D>
__global__ void __launch_bounds__(256) k_jet_matrix(tg_jet_args P) {
  constexpr int NJ = D == 1 ? 3 : 6;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int p1 = P.p + 1, nq = P.nq;
  const int nloc = D == 1 ? p1 : p1 * p1, nqt = D == 1 ? nq : nq * nq;
  double *tl = reinterpret_cast<double *>(smem);
  double *tdl = tl + p1 * nq;
  double *td2 = tdl + p1 * nq + nq;
  double *Tq = td2 + p1 * nq;                      // [nJ^2][nqt]
  const int tid = threadIdx.x, nt = blockDim.x;
  int el[2];
  const int64_t q0g = tg_jet_colour_element<D>(P, el) * nqt;    // first point of the element
  for (int s = tid; s < 3 * p1 * nq + nq; s += nt) tl[s] = P.tab[s];
  for (int s = tid; s < NJ * NJ * nqt; s += nt) {
    const int c = s / nqt, q = s - c * nqt;
    Tq[s] = P.in[(int64_t)c * P.npts + q0g + q];
  }
  __syncthreads();
  for (int pr = tid; pr < nloc * nloc; pr += nt) {
    const int a = pr / nloc, b = pr - a * nloc;
    const int ak[2] = {a % p1, a / p1}, bk[2] = {b % p1, b / p1};
    double acc = 0.0;
    for (int q = 0; q < nqt; q++) {
      double Ja[NJ], Jb[NJ];
      tg_jet_basis<D>(tl, tdl, td2, nq, ak[0], ak[1], q % nq, q / nq, Ja);
      tg_jet_basis<D>(tl, tdl, td2, nq, bk[0], bk[1], q % nq, q / nq, Jb);
      double t = 0.0;
#pragma unroll
      for (int al = 0; al < NJ; al++) {
        double x = 0.0;
#pragma unroll
        for (int be = 0; be < NJ; be++) x = fma(Tq[(al * NJ + be) * nqt + q], Jb[be], x);
        t = fma(Ja[al], x, t);
      }
      acc += t;
    }
    // CSR slot of (row a, col b): the element-coupling pattern, as k_coef_matrix
    int64_t row = 0, rstride = 1;
    int pos = 0, pstride = 1;
#pragma unroll
    for (int k = 0; k < D; k++) {
      const int r = el[k] * P.p + ak[k], c = el[k] * P.p + bk[k];
      int lo, width;
      if (r % P.p == 0) {
        const int l = max(0, r - P.p), h = min(P.n[k] - 1, r + P.p);
        lo = l;
        width = h - l + 1;
      } else {
        lo = (r / P.p) * P.p;
        width = p1;
      }
      row += rstride * r;
      rstride *= P.n[k];
      pos += pstride * (c - lo);
      pstride *= width;
    }
    P.val[P.rowptr[row] + pos] += acc;
  }
}

// out_{i,a} += sum_q sum_alpha s'^alpha_{i,q} J^alpha_ref phi_a for the nblk fields, one after the other
template <int D>
__global__ void __launch_bounds__(256) k_jet_load(tg_jet_args P) {
  constexpr int NJ = D == 1 ? 3 : 6;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int p1 = P.p + 1, nq = P.nq;
  const int nloc = D == 1 ? p1 : p1 * p1, nqt = D == 1 ? nq : nq * nq;
  double *tl = reinterpret_cast<double *>(smem);
  double *tdl = tl + p1 * nq;
  double *td2 = tdl + p1 * nq + nq;
  double *sq = td2 + p1 * nq;                      // [nJ][nqt]
  const int tid = threadIdx.x, nt = blockDim.x;
  int el[2];
  const int64_t q0g = tg_jet_colour_element<D>(P, el) * nqt;
  for (int s = tid; s < 3 * p1 * nq + nq; s += nt) tl[s] = P.tab[s];
  for (int i = 0; i < P.nblk; i++) {
    __syncthreads();                               // (the tables; the previous field's reads)
    for (int s = tid; s < NJ * nqt; s += nt) {
      const int c = s / nqt, q = s - c * nqt;
      sq[s] = P.in[(int64_t)(i * NJ + c) * P.npts + q0g + q];
    }
    __syncthreads();
    for (int a = tid; a < nloc; a += nt) {
      const int a0 = a % p1, a1 = a / p1;
      double acc = 0.0;
      for (int q = 0; q < nqt; q++) {
        double Ja[NJ];
        tg_jet_basis<D>(tl, tdl, td2, nq, a0, a1, q % nq, q / nq, Ja);
        double t = 0.0;
#pragma unroll
        for (int al = 0; al < NJ; al++) t = fma(sq[al * nqt + q], Ja[al], t);
        acc += t;
      }
      const int64_t node = (int64_t)(el[0] * P.p + a0) + (int64_t)P.n[0] * (el[1] * P.p + a1);
      P.out[(int64_t)i * P.nnodes + node] += acc;
    }
  }
}

// ---- host drivers
#define TG_JET_LDS_DEFAULT ((size_t)64 * 1024)     // dynamic LDS of a launch without an attribute

// checks the patch (d = 1, 2), uploads (or keeps) tables and vertices, fills what every kernel shares.  An element needs
// per_elem_of_nc * nc * (p+1)^d + per_elem_fixed doubles of LDS beyond the tables (nc: the nodal fields read; 0 without
// `fields`); `grouped`: a workgroup starts the fit with max(1, 256 / nq^d) elements (k_jet_points), else it takes one
static int tg_jet_setup(const char *who, const tg_patch_t *pt, bool fields, tg_vec_t u, int per_elem_of_nc, int per_elem_fixed,
                        bool grouped, tg_jet_args *A, tg_patch_dims *D, size_t *lds) {
  TG_TRY(tg_patch_check(who, pt, 1, fields, u, D));
  TG_REQUIRE(D->d <= 2, "%s: d = %d; second-derivative point forms are provided for curves and surfaces (d = 1, 2)", who, D->d);
  memset(A, 0, sizeof(*A));
  A->p = D->p, A->nsd = D->nsd, A->nq = D->nq;
  for (int k = 0; k < 3; k++) A->nel[k] = D->nel[k], A->n[k] = D->n[k];
  A->nelem = D->nelem;
  A->npts = D->npts;
  A->nnodes = D->nnodes;
  if (fields) A->nc = tg_point_fields(pt, u, A->f);
  TG_TRY(tg_asm_cache_get(pt));
  A->tab = g_asm_cache.tab;
  for (int k = 0; k < D->d; k++) A->verts[k] = g_asm_cache.verts[k];
  // the tables here are l | dl | w | d2l: (p+1) nq doubles more than tg_point_lds_fit counts
  const int p1 = D->p + 1;
  const size_t extra = (size_t)p1 * D->nq * sizeof(double);
  tg_point_lds_fit(p1, D->nq, per_elem_of_nc * A->nc * D->nloc + per_elem_fixed, 0, grouped ? std::max(1, 256 / D->nqt) : 1,
                   TG_JET_LDS_DEFAULT - extra, &A->epg, lds);
  *lds += extra;
  TG_REQUIRE(*lds <= TG_JET_LDS_DEFAULT, "%s: element data (%zu B) does not fit in LDS", who, *lds);
  TG_REQUIRE(tg_cdiv(D->nelem, A->epg) < (1ll << 31), "%s: too many elements for one launch", who);
  return 0;
}

template <int MODE, bool RAT>
static int tg_jet_points_launch(const tg_jet_args &A, int d, size_t lds) {
  if (A.nelem <= 0) return 0;
  const dim3 grid((unsigned)tg_cdiv(A.nelem, A.epg));
  if (d == 1)
    hipLaunchKernelGGL((k_jet_points<1, MODE, RAT>), grid, dim3(256), lds, g_tg.stream, A);
  else
    hipLaunchKernelGGL((k_jet_points<2, MODE, RAT>), grid, dim3(256), lds, g_tg.stream, A);
  TG_LAUNCH_CHECK();
  return 0;
}

static inline int tg_jet_nj(int d) { return d == 1 ? 3 : 6; }

extern "C" int tg_quad_jet(const tg_patch_t *patch, tg_vec_t u_nodal, int rational, tg_vec_t jet_out) {
  tg_jet_args A;
  tg_patch_dims D;
  size_t lds;
  TG_REQUIRE(u_nodal, "tg_quad_jet: no nodal vector");
  TG_TRY(tg_jet_setup("tg_quad_jet", patch, true, u_nodal, 1, 0, true, &A, &D, &lds));
  TG_REQUIRE(jet_out && jet_out->n == (int64_t)tg_jet_nj(D.d) * D.npts, "tg_quad_jet: an output of nJ npts = %lld values",
             (long long)(tg_jet_nj(D.d) * D.npts));
  A.out = jet_out->d;
  return rational ? tg_jet_points_launch<TG_JET_POINTS_U, true>(A, D.d, lds) : tg_jet_points_launch<TG_JET_POINTS_U, false>(A, D.d, lds);
}

extern "C" int tg_quad_geometry_jet(const tg_patch_t *patch, tg_vec_t jet_out) {
  tg_jet_args A;
  tg_patch_dims D;
  size_t lds;
  TG_TRY(tg_jet_setup("tg_quad_geometry_jet", patch, true, nullptr, 1, 0, true, &A, &D, &lds));
  TG_REQUIRE(jet_out && jet_out->n == (int64_t)D.nsd * tg_jet_nj(D.d) * D.npts,
             "tg_quad_geometry_jet: an output of nsd nJ npts = %lld values", (long long)(D.nsd * tg_jet_nj(D.d) * D.npts));
  A.out = jet_out->d;
  return tg_jet_points_launch<TG_JET_POINTS_GEOM, true>(A, D.d, lds);
}

extern "C" int tg_jet_transform(const tg_patch_t *patch, int rational, int nblk, tg_vec_t T_q, tg_vec_t coef_out) {
  tg_jet_args A;
  tg_patch_dims D;
  size_t lds;
  TG_TRY(tg_jet_setup("tg_jet_transform", patch, true, nullptr, 1, 0, true, &A, &D, &lds));
  const int nJ = tg_jet_nj(D.d);
  TG_REQUIRE(nblk >= 1, "tg_jet_transform: nblk = %d blocks", nblk);
  const int64_t want = (int64_t)nblk * nJ * nJ * D.npts;
  TG_REQUIRE(T_q && T_q->n == want && coef_out && coef_out->n == want && coef_out->d != T_q->d,
             "tg_jet_transform: T_q and a separate output of nblk nJ^2 npts = %lld values each", (long long)want);
  A.nblk = nblk;
  A.in = T_q->d;
  A.out = coef_out->d;
  return rational ? tg_jet_points_launch<TG_JET_POINTS_T, true>(A, D.d, lds) : tg_jet_points_launch<TG_JET_POINTS_T, false>(A, D.d, lds);
}

extern "C" int tg_jet_load_transform(const tg_patch_t *patch, int rational, int nF, tg_vec_t s_q, tg_vec_t out) {
  tg_jet_args A;
  tg_patch_dims D;
  size_t lds;
  TG_TRY(tg_jet_setup("tg_jet_load_transform", patch, true, nullptr, 1, 0, true, &A, &D, &lds));
  TG_REQUIRE(nF >= 1, "tg_jet_load_transform: nF = %d fields", nF);
  const int64_t want = (int64_t)nF * tg_jet_nj(D.d) * D.npts;
  TG_REQUIRE(s_q && s_q->n == want && out && out->n == want && out->d != s_q->d,
             "tg_jet_load_transform: s_q and a separate output of nF nJ npts = %lld values each", (long long)want);
  A.nblk = nF;
  A.in = s_q->d;
  A.out = out->d;
  return rational ? tg_jet_points_launch<TG_JET_POINTS_S, true>(A, D.d, lds) : tg_jet_points_launch<TG_JET_POINTS_S, false>(A, D.d, lds);
}

// one launch per colour of k_jet_matrix / k_jet_load
template <class K1, class K2>
static int tg_jet_coloured(const char *who, tg_jet_args &A, int d, size_t lds, K1 k1, K2 k2) {
  const int rc = tg_for_colours(d, A.nel, [&](const int *efirst, const int *ncol, int64_t nblk) {
    if (nblk >= (1ll << 31)) return 2;
    std::copy_n(efirst, 3, A.efirst);
    std::copy_n(ncol, 3, A.ncol);
    if (d == 1)
      hipLaunchKernelGGL(k1, dim3((unsigned)nblk), dim3(256), lds, g_tg.stream, A);
    else
      hipLaunchKernelGGL(k2, dim3((unsigned)nblk), dim3(256), lds, g_tg.stream, A);
    return hipGetLastError() != hipSuccess ? 1 : 0;
  });
  if (rc == 2) tg_set_error("%s: too many elements for one launch", who);
  if (rc == 1) tg_set_error("%s: the kernel failed to launch", who);
  return rc;
}

extern "C" int tg_assemble_jet_blocks(const tg_patch_t *pt, int nF, tg_vec_t coef, tg_csr_t *out) {
  tg_jet_args A;
  tg_patch_dims D;
  size_t lds;
  TG_REQUIRE(pt && out, "tg_assemble_jet_blocks: null patch or output");
  const int nJ = tg_jet_nj(pt->d);
  TG_REQUIRE(pt->nq >= 1 && pt->nq <= TG_ASM_MAXQ1, "tg_assemble_jet_blocks: 1..%d Gauss points per direction", TG_ASM_MAXQ1);
  TG_TRY(tg_jet_setup("tg_assemble_jet_blocks", pt, false, nullptr, 0, nJ * nJ * tg_ipow(pt->nq, pt->d == 1 ? 1 : 2), false, &A, &D,
                      &lds));                      // (the control functions are not read)
  TG_REQUIRE(nF >= 1, "tg_assemble_jet_blocks: nF = %d fields", nF);
  const int64_t each = (int64_t)nJ * nJ * D.npts, nb = (int64_t)nF * nF;
  TG_REQUIRE(coef && coef->n == nb * each, "tg_assemble_jet_blocks: nF^2 nJ^2 npts = %lld transformed point values (tg_jet_transform)",
             (long long)(nb * each));
  std::vector<tg_csr_t> blocks((size_t)nb, nullptr);
  const bool timeit = getenv("TIGAR_ASM_TIME") != nullptr;
  int rc = 0;
  for (int64_t b = 0; b < nb && !rc; b++) {
    rc = tg_asm_coupling_pattern(D.d, D.p, A.n, 0, D.nnodes, false, &blocks[b]);    // (values 0: the colours add into them)
    if (rc) break;
    A.in = coef->d + b * each;
    A.rowptr = blocks[b]->rowptr;
    A.val = blocks[b]->val;
    if (timeit) hipEventRecord(g_tg.ev0[0], g_tg.stream);
    rc = tg_jet_coloured("tg_assemble_jet_blocks", A, D.d, lds, k_jet_matrix<1>, k_jet_matrix<2>);
    if (timeit && !rc) {
      hipEventRecord(g_tg.ev1[0], g_tg.stream);
      hipEventSynchronize(g_tg.ev1[0]);
      float ms = 0.f;
      hipEventElapsedTime(&ms, g_tg.ev0[0], g_tg.ev1[0]);
      fprintf(stderr, "[tg_assemble] jet form, block %lld of %lld, %lld points: element kernels %.3f ms (plain)\n", (long long)b,
              (long long)nb, (long long)D.npts, ms);
    }
  }
  if (!rc) {
    if (nF == 1) {
      *out = blocks[0];
      blocks[0] = nullptr;
    } else {
      rc = tg_csr_from_blocks(nF, blocks.data(), out);
    }
  }
  for (tg_csr_t b : blocks)
    if (b) tg_csr_destroy(b);
  return rc;
}

extern "C" int tg_quad_load_jet(const tg_patch_t *pt, int nF, tg_vec_t s_t, tg_vec_t out) {
  tg_jet_args A;
  tg_patch_dims D;
  size_t lds;
  TG_REQUIRE(pt, "tg_quad_load_jet: null patch");
  const int nJ = tg_jet_nj(pt->d);
  TG_REQUIRE(pt->nq >= 1 && pt->nq <= TG_ASM_MAXQ1, "tg_quad_load_jet: 1..%d Gauss points per direction", TG_ASM_MAXQ1);
  TG_TRY(tg_jet_setup("tg_quad_load_jet", pt, false, nullptr, 0, nJ * tg_ipow(pt->nq, pt->d == 1 ? 1 : 2), false, &A, &D, &lds));
  TG_REQUIRE(nF >= 1, "tg_quad_load_jet: nF = %d fields", nF);
  TG_REQUIRE(s_t && s_t->n == (int64_t)nF * nJ * D.npts, "tg_quad_load_jet: nF nJ npts = %lld transformed point values (tg_jet_load_transform)",
             (long long)(nF * nJ * D.npts));
  A.nblk = nF;
  A.in = s_t->d;
  TG_TRY(tg_point_nodal_output("tg_quad_load_jet", out, (int64_t)nF * D.nnodes, &A.out));     // (nF fields, one after the other)
  return tg_jet_coloured("tg_quad_load_jet", A, D.d, lds, k_jet_load<1>, k_jet_load<2>);
}
