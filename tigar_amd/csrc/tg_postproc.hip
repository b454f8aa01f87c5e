// Quadrature-point evaluation on mapped tensor-product patches: what a caller needs around the solve -- L2 projection of a
// function onto the spline space (initial and boundary data), and the error of a computed solution against an exact one
// (tIGAr/common.py:1392-1433 project; the demos' sqrt(assemble(((u-soln)**2)*spline.dx))).
//
// Scalar Q_p Lagrange space on the tensor node grid, geometry F = cp[i]/cp[nsd], Gauss-Legendre with nq points per
// direction: the conventions of tg_assemble.hip.  Points are numbered element-major (elements lexicographic with
// direction 0 fastest, the nq^d points of an element likewise); point arrays with several components are component-major.
//
//   tg_quad_points   x_q = F(xi_q) and wdet_q = w_q sqrt(det g) prod h_k
//   tg_quad_eval     u_h(x_q) and the Cartesian gradient DF g^-1 grad_xi u_h (pinv(DF), quotient rule of the rational map)
//   tg_quad_load     out[node] = sum_q wdet_q f_q phi_node(xi_q)
//   tg_quad_error    sum wdet (u_h - e)^2,  sum wdet |grad u_h - ge|^2,  sum wdet e^2
//   tg_coef_transform / tg_flux_transform   Cartesian point coefficients -> the reference element (formulas: tg_coef.hip)
//   tg_coef_transform_blocks   the same for the nF^2 blocks of a vector-valued unknown's tangent, the geometry formed once
//   tg_coef_transform_system   ... for the nF^2 blocks of a first-order system: every block with its own A, b, c and m
//   tg_quad_metric   G = 4 P P^T, P = DF g^-1: the element metric of the bi-unit parent element (stabilisation parameters)
//   tg_quad_load_flux   out[node] = sum_q wdet_q (s_q phi_node + F_q . grad phi_node)(xi_q)
//   tg_lattice_points / tg_lattice_eval   endings 0 and 1 on the tensor lattice of m abscissae the caller gives per element
//                       (output for a viewer, sampling on a regular grid): the host builds l | dl there in the place of the Gauss table
//
// One kernel, four endings (and the three that take point coefficients).  A workgroup of 256 threads takes max(1, 256 / nq^d) elements (fewer where
// their LDS areas would exceed 64 KiB).  The nodal values of the
// nsd + 1 control functions (and of u) go to the points by SUM FACTORISATION: one 1-D contraction per direction through
// LDS, O((p+1) nq^d) per field instead of the O((p+1)^d nq^d) of the plain assembly kernel; the load goes back to the
// nodes the same way.  Everything is done in the coordinates of the reference element [0,1]^d: DF, g and the gradients
// of the Lagrange functions refer to them, so that no element size appears -- w_q sqrt(det g_hat) IS w_q sqrt(det g)
// prod h_k, and DF g^-1 grad u is the same vector in any parametrisation (tIGAr/calculusUtils.py:56-70).
// No floating-point atomics: the load adds element by element, colour by colour (parities of the element index, the
// colours of k_assemble_mapped in the same order); the error sums are per-element trees, then one fixed pass over the
// elements.  Same inputs, same bits.
//
// RATIONAL functions (u = u_h / W_h, the reference's spline.rationalize(u); tested against phi / W_h): W_h and its gradient
// are at the points anyway --  u = u_h / W_h,  grad_xi u = (grad_xi u_h - u grad_xi W_h) / W_h  before the Cartesian
// gradient and the error terms are formed, and the load's point value takes 1 / W_h.
//
// The check of the patch, the LDS fit, the colour loop and the nodal fields' has / ci are tg_point_shared.h's, shared with
// tg_boundary.hip and tg_coef.hip.
#include "tg_common.h"
#include "tg_point_shared.h"
#include <cmath>

struct tg_pp_args {
  int d, p, nsd, nq;
  int nel[3], n[3];            // elements / nodes per direction (1 beyond d)
  const double *f[5];          // nodal fields: 0..2 homogeneous coordinates (the first nsd), 3 the weight function, 4 u (or null)
  int nc;                      // how many of them there are
  const double *tab;           // l[a][q] | dl[a][q] | w[q]
  int epg;                     // elements per workgroup
  int szA, szB;                // doubles per element of the two LDS areas
  int efirst[3], ncol[3], estep;   // the elements of this launch: efirst[k] + estep i, i < ncol[k]
  int64_t nelem;               // ... their number
  int64_t npts;                // points of the patch
  double *x, *wdet;            // points
  double *val, *grad;          // eval (grad may be null)
  const double *fq;            // load: point values
  double *out;                 //       nodal vector
  const double *eq, *geq;      // error: point values of e and of its gradient (either may be null)
  double *part;                //        [3][elements of the patch] partial sums
  // point coefficients (TG_PP_COEF, TG_PP_FLUX): Cartesian data at the points, any of them null = 0
  int akind;                   // diffusion: 0 none, 1 one value per point, 2 an nsd x nsd tensor per point
  const double *Aq, *bq, *cq, *mq;   // a(u, v) = int grad v . (A grad u) + (b . grad v) u + v (c . grad u) + m u v
  const double *sq, *Fq;       // L(v) = int s v + F . grad v
  double *cout;                // the data on the reference element, component-major
  int nblk;                    // TG_PP_BLOCKS: Aq, bq, cq, mq and cout hold this many consecutive sets (a tensor, two vectors
                               // and a value per point each; any of the four may be null)
};

// element number e of the launch -> element indices; returns the lexicographic index in the patch
__device__ __forceinline__ int64_t tg_pp_element(const tg_pp_args &P, int64_t e, int *el) {
  el[0] = P.efirst[0] + P.estep * (int)(e % P.ncol[0]);
  e /= P.ncol[0];
  el[1] = P.efirst[1] + P.estep * (int)(e % P.ncol[1]);
  e /= P.ncol[1];
  el[2] = P.efirst[2] + P.estep * (int)e;
  return (int64_t)el[0] + (int64_t)P.nel[0] * ((int64_t)el[1] + (int64_t)P.nel[1] * el[2]);
}

__device__ __forceinline__ int64_t tg_pp_node(const tg_pp_args &P, const int *el, int a) {
  const int p1 = P.p + 1;
  const int a0 = a % p1, a1 = (a / p1) % p1, a2 = a / (p1 * p1);
  return (int64_t)(el[0] * P.p + a0) + (int64_t)P.n[0] * ((int64_t)(el[1] * P.p + a1) + (int64_t)P.n[1] * (el[2] * P.p + a2));
}

// MODE 0 points, 1 eval, 2 load, 3 error; + 4 (TG_PP_RAT): rational functions (eval, load, error)
// Point coefficients (tg_coef.hip has the formulas): 0 + TG_PP_COEF writes the d^2 + 2d + 1 reference-element coefficients
// of the matrix form in the place of the points, 0 + TG_PP_FLUX the d + 1 of the load; 2 + TG_PP_FLUX is the load of
// s v + F . grad v.  All three take TG_PP_RAT: beta is folded into the data.  TG_PP_COEF + TG_PP_BLOCKS: the coefficient ending
// looped over nblk sets of (tensor, reaction) -- the nF^2 blocks of a vector-valued unknown's tangent (tg_material.hip) --
// with the point's geometry (P = DF g^-1, wdet, W, beta) computed once.  0 + TG_PP_METRIC writes G = 4 P P^T (nsd x nsd) in
// the place of the points.
#define TG_PP_RAT 4
#define TG_PP_COEF 8
#define TG_PP_FLUX 16
#define TG_PP_BLOCKS 32
#define TG_PP_METRIC 64
template <int MODER>
__global__ void __launch_bounds__(256) k_postproc(tg_pp_args P) {
  constexpr int MODE = MODER & 3;
  constexpr bool RAT = (MODER & TG_PP_RAT) != 0;
  constexpr bool COEF = (MODER & TG_PP_COEF) != 0, FLUX = (MODER & TG_PP_FLUX) != 0, BLK = (MODER & TG_PP_BLOCKS) != 0;
  constexpr bool METRIC = (MODER & TG_PP_METRIC) != 0;
  static_assert(!BLK || COEF, "the blocks are sets of point coefficients");
  static_assert(!METRIC || MODER == TG_PP_METRIC, "the metric is a property of the points");
  static_assert(!(RAT && MODE == 0 && !COEF && !FLUX), "the points do not depend on the function space");
  static_assert(!(COEF && (MODE != 0 || FLUX)) && !(FLUX && MODE != 0 && MODE != 2), "endings that take point coefficients");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int d = P.d, p1 = P.p + 1, nq = P.nq, nsd = P.nsd, nc = P.nc, epg = P.epg;
  const int nloc = d == 1 ? p1 : (d == 2 ? p1 * p1 : p1 * p1 * p1);
  const int nqt = d == 1 ? nq : (d == 2 ? nq * nq : nq * nq * nq);
  double *tl = reinterpret_cast<double *>(smem);   // l[a][q]
  double *tdl = tl + p1 * nq;                      // dl[a][q]
  double *tw = tdl + p1 * nq;                      // w[q]
  double *bufA = tw + nq;
  double *bufB = bufA + (size_t)epg * P.szA;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t g0 = (int64_t)blockIdx.x * epg;    // first element of the group (of this launch's elements)
  for (int s = tid; s < 2 * p1 * nq + nq; s += nt) tl[s] = P.tab[s];
  // nodal values -> area A [field][local node]
  for (int i = tid; i < epg * nloc; i += nt) {
    const int es = i / nloc, a = i - es * nloc;
    if (g0 + es >= P.nelem) continue;
    int el[3];
    tg_pp_element(P, g0 + es, el);
    const int64_t node = tg_pp_node(P, el, a);
#pragma unroll
    for (int c = 0; c < 5; c++)
      if (tg_pt_has(c, nsd, P.f)) bufA[(size_t)es * P.szA + tg_pt_ci(c, nsd) * nloc + a] = P.f[c][node];
  }
  __syncthreads();
  // ---- to the points: directions 0 .. d-2 through LDS.  Before direction k an area holds k + 1 "slots" per field --
  // the function and its derivatives in the directions done -- on [q_0 .. q_k-1 | a_k .. a_d-1]; the contraction with
  // l gives each slot on [q_0 .. q_k | a_k+1 ..], the contraction of the function with dl the new derivative.
  // Layout: area[(slot nc + field) S + index].
  int nqk = 1, rest = nloc / p1;                   // nq^k, (p+1)^(d-k-1)
  for (int k = 0; k + 1 < d; k++) {
    const double *in = (k & 1) ? bufB : bufA;
    double *out = (k & 1) ? bufA : bufB;
    const int szi = (k & 1) ? P.szB : P.szA, szo = (k & 1) ? P.szA : P.szB;
    const int Sin = nqk * p1 * rest, Sout = nqk * nq * rest, work = nc * Sout;
    for (int i = tid; i < epg * work; i += nt) {
      const int es = i / work, r = i - es * work;
      if (g0 + es >= P.nelem) continue;
      const int ci = r / Sout, idx = r - ci * Sout;
      const int Q = idx % nqk, t = idx / nqk, qk = t % nq, R = t / nq;
      const double *I = in + (size_t)es * szi + ci * Sin;
      double v0 = 0.0, v1 = 0.0, vd = 0.0;
      for (int a = 0; a < p1; a++) {
        const double l = tl[a * nq + qk], dl = tdl[a * nq + qk];
        const int off = Q + nqk * (a + p1 * R);
        const double f0 = I[off];
        v0 = fma(l, f0, v0);
        vd = fma(dl, f0, vd);
        if (k >= 1) v1 = fma(l, I[nc * Sin + off], v1);
      }
      double *O = out + (size_t)es * szo + ci * Sout;
      O[idx] = v0;
      if (k >= 1) O[nc * Sout + idx] = v1;
      O[(k + 1) * nc * Sout + idx] = vd;
    }
    __syncthreads();
    nqk *= nq;
    rest /= p1;
  }
  // ---- the last direction: a thread per point, results in registers
  const bool lastB = ((d - 1) & 1) != 0;           // the area the last contraction reads; the OTHER one is free
  const double *fin = lastB ? bufB : bufA;
  double *oth = lastB ? bufA : bufB;
  const int szf = lastB ? P.szB : P.szA, szt = lastB ? P.szA : P.szB;
  const int Sin = nqk * p1;
  for (int i = tid; i < epg * nqt; i += nt) {
    const int es = i / nqt, q = i - es * nqt;
    if (g0 + es >= P.nelem) continue;
    const int Q = q % nqk, ql = q / nqk;
    double N[5], dN[5][3];
#pragma unroll
    for (int c = 0; c < 5; c++) {
      N[c] = 0.0;
      dN[c][0] = dN[c][1] = dN[c][2] = 0.0;
      if (!tg_pt_has(c, nsd, P.f)) continue;
      const double *I = fin + (size_t)es * szf + tg_pt_ci(c, nsd) * Sin;
      double v = 0.0, e0 = 0.0, e1 = 0.0, vd = 0.0;
      for (int a = 0; a < p1; a++) {
        const double l = tl[a * nq + ql], dl = tdl[a * nq + ql];
        const int off = Q + nqk * a;
        const double f0 = I[off];
        v = fma(l, f0, v);
        vd = fma(dl, f0, vd);
        if (d >= 2) e0 = fma(l, I[nc * Sin + off], e0);
        if (d >= 3) e1 = fma(l, I[2 * nc * Sin + off], e1);
      }
      N[c] = v;
      dN[c][0] = d == 1 ? vd : e0;
      dN[c][1] = d == 2 ? vd : e1;
      dN[c][2] = d == 3 ? vd : 0.0;
    }
    // DF[i][k] = d(N_i / W)/dxi_k ; metric g = DF^T DF  (the twin of quotient, DF and g: k_boundary, tg_boundary.hip)
    const double W = N[3];
    if constexpr (RAT && (MODE == 1 || MODE == 3)) {
      // the difference first, with one rounding (for a function of the space the two products nearly cancel), then the division
      const double rw = 1.0 / W;
#pragma unroll
      for (int k = 0; k < 3; k++) dN[4][k] = fma(dN[4][k], W, -(N[4] * dN[3][k])) * (rw * rw);
      N[4] *= rw;
    }
    double G[3][3], DF[3][3] = {{0}};
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (c >= nsd) continue;
#pragma unroll
      for (int k = 0; k < 3; k++)
        if (k < d) DF[c][k] = (dN[c][k] * W - N[c] * dN[3][k]) / (W * W);
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int m = 0; m < 3; m++) G[k][m] = DF[0][k] * DF[0][m] + DF[1][k] * DF[1][m] + DF[2][k] * DF[2][m];   // (zero beyond nsd, d)
    double gi[3][3];
    const double det = tg_point_metric_inverse<true>(d, G, gi);
    const int q0 = q % nq, q1 = (q / nq) % nq, q2 = q / (nq * nq);
    const double wq = tw[q0] * (d > 1 ? tw[q1] : 1.0) * (d > 2 ? tw[q2] : 1.0);
    const double wdet = wq * sqrt(fabs(det));
    // Cartesian gradient of u: DF g^-1 grad_xi u
    double gu[3] = {0, 0, 0};
    if (MODE == 1 || MODE == 3) {
      double t[3];
#pragma unroll
      for (int k = 0; k < 3; k++) t[k] = gi[k][0] * dN[4][0] + gi[k][1] * dN[4][1] + gi[k][2] * dN[4][2];
#pragma unroll
      for (int c = 0; c < 3; c++) gu[c] = DF[c][0] * t[0] + DF[c][1] * t[1] + DF[c][2] * t[2];
    }
    int el[3];
    const int64_t gp = tg_pp_element(P, g0 + es, el) * nqt + q;    // the point's number in the patch
    if constexpr (COEF || FLUX) {
      // Cartesian data -> reference element: P = DF g^-1 (nsd x d; zero beyond), beta = grad_xi W_h / W_h
      double Pm[3][3], bt[3];
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 3; k++) Pm[c][k] = DF[c][0] * gi[0][k] + DF[c][1] * gi[1][k] + DF[c][2] * gi[2][k];
#pragma unroll
      for (int k = 0; k < 3; k++) bt[k] = RAT ? dN[3][k] / W : 0.0;
      [[maybe_unused]] const double rw = 1.0 / W;
      if constexpr (COEF) {
        const int nblk = BLK ? P.nblk : 1;
        for (int blk = 0; blk < nblk; blk++) {
          const double *Aq = P.Aq, *bq = P.bq, *cq = P.cq, *mq = P.mq;
          double *co = P.cout;
          if constexpr (BLK) {           // set blk: an nsd x nsd tensor, two nsd-vectors and a reaction value per point, each optional
            if (Aq) Aq += (int64_t)blk * nsd * nsd * P.npts;
            if (bq) bq += (int64_t)blk * nsd * P.npts;
            if (cq) cq += (int64_t)blk * nsd * P.npts;
            if (mq) mq += (int64_t)blk * P.npts;
            co += (int64_t)blk * (d * d + 2 * d + 1) * P.npts;
          }
          double Ch[3][3] = {{0}}, bh[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, mh = 0.0;
          if (P.akind == 1) {            // P^T P = g^-1
            const double a = wdet * Aq[gp];
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
              for (int m = 0; m < 3; m++) Ch[k][m] = a * gi[k][m];
          } else if (P.akind == 2) {
            double T[3][3] = {{0}};      // A P
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
              for (int e = 0; e < 3; e++) {
                if (c >= nsd || e >= nsd) continue;
                const double a = Aq[(int64_t)(c * nsd + e) * P.npts + gp];
#pragma unroll
                for (int m = 0; m < 3; m++) T[c][m] = fma(a, Pm[e][m], T[c][m]);
              }
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
              for (int m = 0; m < 3; m++) Ch[k][m] = wdet * (Pm[0][k] * T[0][m] + Pm[1][k] * T[1][m] + Pm[2][k] * T[2][m]);
          }
#pragma unroll
          for (int c = 0; c < 3; c++) {
            if (c >= nsd) continue;
            const double bc = bq ? wdet * bq[(int64_t)c * P.npts + gp] : 0.0;
            const double cc = cq ? wdet * cq[(int64_t)c * P.npts + gp] : 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
              bh[k] = fma(Pm[c][k], bc, bh[k]);
              ch[k] = fma(Pm[c][k], cc, ch[k]);
            }
          }
          if (mq) mh = wdet * mq[gp];
          if constexpr (RAT) {
            // psi = phi / W, grad_xi psi = (grad_xi phi - phi beta) / W: everything takes 1 / W^2, then the terms with beta move
            // from the tensor to the vectors and from the vectors to the scalar
            const double rw2 = rw * rw;
            double Cb[3], Ctb[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
#pragma unroll
              for (int m = 0; m < 3; m++) Ch[k][m] *= rw2;
              bh[k] *= rw2;
              ch[k] *= rw2;
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
              Cb[k] = Ch[k][0] * bt[0] + Ch[k][1] * bt[1] + Ch[k][2] * bt[2];
              Ctb[k] = Ch[0][k] * bt[0] + Ch[1][k] * bt[1] + Ch[2][k] * bt[2];
            }
            mh = mh * rw2 - (bt[0] * bh[0] + bt[1] * bh[1] + bt[2] * bh[2]) - (bt[0] * ch[0] + bt[1] * ch[1] + bt[2] * ch[2]) +
                 (bt[0] * Cb[0] + bt[1] * Cb[1] + bt[2] * Cb[2]);
#pragma unroll
            for (int k = 0; k < 3; k++) {
              bh[k] -= Cb[k];
              ch[k] -= Ctb[k];
            }
          }
          double *o = co + gp;           // C (row-major d x d) | b | c | m
#pragma unroll
          for (int k = 0; k < 3; k++)
#pragma unroll
            for (int m = 0; m < 3; m++)
              if (k < d && m < d) o[(int64_t)(k * d + m) * P.npts] = Ch[k][m];
#pragma unroll
          for (int k = 0; k < 3; k++)
            if (k < d) {
              o[(int64_t)(d * d + k) * P.npts] = bh[k];
              o[(int64_t)(d * d + d + k) * P.npts] = ch[k];
            }
          o[(int64_t)(d * d + 2 * d) * P.npts] = mh;
        }
      } else {
        double sh = P.sq ? wdet * P.sq[gp] : 0.0, Fh[3] = {0, 0, 0};
        if (P.Fq) {
#pragma unroll
          for (int c = 0; c < 3; c++) {
            if (c >= nsd) continue;
            const double fc = wdet * P.Fq[(int64_t)c * P.npts + gp];
#pragma unroll
            for (int k = 0; k < 3; k++) Fh[k] = fma(Pm[c][k], fc, Fh[k]);
          }
        }
        if constexpr (RAT) {
          sh = (sh - (Fh[0] * bt[0] + Fh[1] * bt[1] + Fh[2] * bt[2])) * rw;
#pragma unroll
          for (int k = 0; k < 3; k++) Fh[k] *= rw;
        }
        // s | F: to memory, or to the slots of the way back to the nodes
        if (MODE == 0) {
          P.cout[gp] = sh;
#pragma unroll
          for (int k = 0; k < 3; k++)
            if (k < d) P.cout[(int64_t)(1 + k) * P.npts + gp] = Fh[k];
        } else {
          double *T = oth + (size_t)es * szt;
          T[q] = sh;
#pragma unroll
          for (int k = 0; k < 3; k++)
            if (k < d) T[(1 + k) * nqt + q] = Fh[k];
        }
      }
    } else if constexpr (METRIC) {
      // d xi' / d x of the bi-unit parent element xi' = 2 xi - 1 is 2 P^T: G_KL = 4 sum_k P_Kk P_Lk, symmetric, all nsd^2 stored
      double Pm[3][3];
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 3; k++) Pm[c][k] = DF[c][0] * gi[0][k] + DF[c][1] * gi[1][k] + DF[c][2] * gi[2][k];
#pragma unroll
      for (int K = 0; K < 3; K++)
#pragma unroll
        for (int L = 0; L < 3; L++)
          if (K < nsd && L < nsd)
            P.cout[(int64_t)(K * nsd + L) * P.npts + gp] = 4.0 * (Pm[K][0] * Pm[L][0] + Pm[K][1] * Pm[L][1] + Pm[K][2] * Pm[L][2]);
    } else if (MODE == 0) {
#pragma unroll
      for (int c = 0; c < 3; c++)
        if (c < nsd) P.x[(int64_t)c * P.npts + gp] = N[c] / W;
      P.wdet[gp] = wdet;
    } else if (MODE == 1) {
      P.val[gp] = N[4];
      if (P.grad) {
#pragma unroll
        for (int c = 0; c < 3; c++)
          if (c < nsd) P.grad[(int64_t)c * P.npts + gp] = gu[c];
      }
    } else if (MODE == 2) {
      oth[(size_t)es * szt + q] = RAT ? wdet * P.fq[gp] / W : wdet * P.fq[gp];
    } else {
      const double e = P.eq ? P.eq[gp] : 0.0;
      const double du = N[4] - e;
      double s1 = 0.0;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        if (c >= nsd) continue;
        const double dg = gu[c] - (P.geq ? P.geq[(int64_t)c * P.npts + gp] : 0.0);
        s1 = fma(dg, dg, s1);
      }
      double *T = oth + (size_t)es * szt;
      T[q] = wdet * (du * du);
      T[nqt + q] = wdet * s1;
      T[2 * nqt + q] = wdet * (e * e);
    }
  }
  if (MODE == 0 || MODE == 1) return;      // (the transforms of the point coefficients are MODE 0)
  __syncthreads();
  if (MODE == 3) {
    // the three sums of each element: a tree over its points (fixed shape), then one value per element and term
    int p2 = 1;
    while (p2 < nqt) p2 <<= 1;
    for (int o = p2 >> 1; o > 0; o >>= 1) {
      for (int i = tid; i < epg * 3 * o; i += nt) {
        const int es = i / (3 * o), r = i - es * 3 * o, t = r / o, j = r - t * o;
        if (j + o < nqt) oth[(size_t)es * szt + t * nqt + j] += oth[(size_t)es * szt + t * nqt + j + o];
      }
      __syncthreads();
    }
    for (int i = tid; i < epg * 3; i += nt) {
      const int es = i / 3, t = i - es * 3;
      if (g0 + es >= P.nelem) continue;
      int el[3];
      const int64_t ei = tg_pp_element(P, g0 + es, el);
      P.part[(int64_t)t * P.nelem + ei] = oth[(size_t)es * szt + t * nqt];
    }
    return;
  }
  // ---- load: wdet f back to the nodes, direction by direction.  Before direction k: [a_0 .. a_k-1 | q_k .. q_d-1]
  double *cur = oth, *nxt = lastB ? bufB : bufA;
  int szc = szt, szn = szf;
  int pk = 1, qrest = nqt / nq;                    // (p+1)^k, nq^(d-k-1)
  for (int k = 0; k < d; k++) {
    const int Sout = pk * p1 * qrest;
    if constexpr (FLUX) {
      // d - k + 1 slots come in: the sum so far, whose remaining tables are all l, and F_k .. F_d-1, each waiting for dl in
      // its own direction.  Direction k contracts F_k with dl into the sum; the others pass with l: d - k slots go out
      const int Sin = pk * nq * qrest, nso = d - k;
      for (int i = tid; i < epg * nso * Sout; i += nt) {
        const int es = i / (nso * Sout), r = i - es * nso * Sout, sl = r / Sout, idx = r - sl * Sout;
        if (g0 + es >= P.nelem) continue;
        const int Ai = idx % pk, t = idx / pk, ak = t % p1, R = t / p1;
        const double *I = cur + (size_t)es * szc + (sl == 0 ? 0 : (sl + 1) * Sin);
        double acc = 0.0;
        for (int q = 0; q < nq; q++) acc = fma(tl[ak * nq + q], I[Ai + pk * (q + nq * R)], acc);
        if (sl == 0)
          for (int q = 0; q < nq; q++) acc = fma(tdl[ak * nq + q], I[Sin + Ai + pk * (q + nq * R)], acc);
        nxt[(size_t)es * szn + sl * Sout + idx] = acc;
      }
    } else {
      for (int i = tid; i < epg * Sout; i += nt) {
        const int es = i / Sout, idx = i - es * Sout;
        if (g0 + es >= P.nelem) continue;
        const int Ai = idx % pk, t = idx / pk, ak = t % p1, R = t / p1;
        const double *I = cur + (size_t)es * szc;
        double acc = 0.0;
        for (int q = 0; q < nq; q++) acc = fma(tl[ak * nq + q], I[Ai + pk * (q + nq * R)], acc);
        nxt[(size_t)es * szn + idx] = acc;
      }
    }
    __syncthreads();
    double *sw = cur;
    cur = nxt;
    nxt = sw;
    const int si = szc;
    szc = szn;
    szn = si;
    pk *= p1;
    qrest /= nq;
  }
  // elements of one launch share no node (one colour): plain adds, the colours follow each other in a fixed order
  for (int i = tid; i < epg * nloc; i += nt) {
    const int es = i / nloc, a = i - es * nloc;
    if (g0 + es >= P.nelem) continue;
    int el[3];
    tg_pp_element(P, g0 + es, el);
    P.out[tg_pp_node(P, el, a)] += cur[(size_t)es * szc + a];
  }
}

// one workgroup per term: thread t adds the elements t, t + 256, ... in that order, then the tree of the workgroup
__global__ void __launch_bounds__(256) k_postproc_fold(const double *part, int64_t nelem, double *out) {
  __shared__ double s[256];
  const double *v = part + (int64_t)blockIdx.x * nelem;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < nelem; i += 256) acc += v[i];
  const double r = tg_block_sum_ordered(acc, s);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}

#define TG_PP_LDS_DEFAULT ((size_t)64 * 1024)     // dynamic LDS of a launch without an attribute
#define TG_PP_LDS_MAX ((size_t)160 * 1024)        // LDS of a compute unit

// checks the patch, fills what every mode shares; `u`: the nodal vector taken to the points (may be null).  mode: 0 - 3 as
// the kernel's, 4 the flux load
static int tg_pp_setup(const char *who, const tg_patch_t *pt, int mode, tg_vec_t u, tg_pp_args *A, size_t *lds,
                       int64_t *nnodes_out = nullptr, bool gauss_tables = true) {
  tg_patch_dims D;
  TG_TRY(tg_patch_check(who, pt, 1, true, u, &D));
  const int d = D.d, p1 = D.p + 1, nq = D.nq, nloc = D.nloc, nqt = D.nqt;
  tg_point_args_init(D, A);
  std::copy_n(D.nel, 3, A->ncol);
  A->estep = 1;
  A->nelem = D.nelem;
  A->npts = D.npts;
  A->nc = tg_point_fields(pt, u, A->f);
  if (nnodes_out) *nnodes_out = D.nnodes;
  if (gauss_tables) {              // (the lattice entries bring their own table)
    TG_TRY(tg_asm_cache_get(pt));
    A->tab = g_asm_cache.tab;
  }
  // LDS per element: area A holds the nodal values, then (3-D) the output of direction 1; area B the output of direction
  // 0; the area the last contraction does not read takes the point values of the load / the terms of the error sums, and
  // the load goes back to the nodes through both
  const int nc = A->nc;
  int szA = nc * nloc, szB = 0;
  if (d >= 2) szB = 2 * nc * nq * (nloc / p1);
  if (d == 3) szA = std::max(szA, 3 * nc * nq * nq * p1);
  const int back = tg_ipow(std::max(p1, nq), d);
  int &other = ((d - 1) & 1) ? szA : szB;
  if (mode == 2) {
    szA = std::max(szA, back);
    szB = std::max(szB, back);
  }
  if (mode == 4) {     // the flux load goes back with up to d + 1 slots
    szA = std::max(szA, (d + 1) * back);
    szB = std::max(szB, (d + 1) * back);
  }
  if (mode == 3) other = std::max(other, 3 * nqt);
  A->szA = szA;
  A->szB = szB;
  // fewer elements per workgroup until the group fits the 64 KiB a launch gets without asking (nq < p + 1: many points'
  // worth of threads, but the areas grow with the nodes); one element of the largest shapes (3-D, p = 4, nq >= 9: 84 KB)
  // needs more than that and asks for it (tg_pp_launch)
  tg_point_lds_fit(p1, nq, szA, szB, std::max(1, 256 / nqt), TG_PP_LDS_DEFAULT, &A->epg, lds);
  TG_REQUIRE(*lds <= TG_PP_LDS_MAX, "%s: element data (%zu B) does not fit in LDS", who, *lds);
  TG_REQUIRE(tg_cdiv(D.nelem, A->epg) < (1ll << 31), "%s: too many elements for one launch", who);
  return 0;
}

template <int MODE>
static int tg_pp_launch(const tg_pp_args &A, size_t lds) {
  if (A.nelem <= 0) return 0;
  if (lds > TG_PP_LDS_DEFAULT)
    TG_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_postproc<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)TG_PP_LDS_MAX));
  hipLaunchKernelGGL((k_postproc<MODE>), dim3((unsigned)tg_cdiv(A.nelem, A.epg)), dim3(256), lds, g_tg.stream, A);
  TG_LAUNCH_CHECK();
  return 0;
}

// the endings that add into the nodes (MODE 2) take one launch per colour, the others one launch; plain or rational
template <int M>
static int tg_pp_launch_rat(bool rat, tg_pp_args &A, size_t lds) {
  auto launch = [&] { return rat ? tg_pp_launch<M | TG_PP_RAT>(A, lds) : tg_pp_launch<M>(A, lds); };
  if ((M & 3) != 2) return launch();
  A.estep = 2;
  return tg_for_colours(A.d, A.nel, [&](const int *efirst, const int *ncol, int64_t count) {
    std::copy_n(efirst, 3, A.efirst);
    std::copy_n(ncol, 3, A.ncol);
    A.nelem = count;
    return launch();
  });
}

extern "C" int tg_quad_points(const tg_patch_t *patch, tg_vec_t x_out, tg_vec_t wdet_out) {
  tg_pp_args A;
  size_t lds;
  TG_TRY(tg_pp_setup("tg_quad_points", patch, 0, nullptr, &A, &lds));
  TG_REQUIRE(x_out && x_out->n == (int64_t)A.nsd * A.npts && wdet_out && wdet_out->n == A.npts,
             "tg_quad_points: outputs of nsd * npts = %lld and npts = %lld values", (long long)(A.nsd * A.npts), (long long)A.npts);
  A.x = x_out->d;
  A.wdet = wdet_out->d;
  return tg_pp_launch<0>(A, lds);
}

static int tg_pp_eval(const tg_patch_t *patch, tg_vec_t u_nodal, int with_grad, tg_vec_t val_out, tg_vec_t grad_out, bool rat) {
  tg_pp_args A;
  size_t lds;
  TG_REQUIRE(u_nodal, "tg_quad_eval: no nodal vector");
  TG_TRY(tg_pp_setup("tg_quad_eval", patch, 1, u_nodal, &A, &lds));
  TG_REQUIRE(val_out && val_out->n == A.npts, "tg_quad_eval: an output of npts = %lld values", (long long)A.npts);
  A.val = val_out->d;
  if (with_grad) {
    TG_REQUIRE(grad_out && grad_out->n == (int64_t)A.nsd * A.npts, "tg_quad_eval: a gradient output of nsd * npts = %lld values",
               (long long)(A.nsd * A.npts));
    A.grad = grad_out->d;
  }
  return tg_pp_launch_rat<1>(rat, A, lds);
}

static int tg_pp_load(const tg_patch_t *patch, tg_vec_t f_q, tg_vec_t out, bool rat) {
  tg_pp_args A;
  size_t lds;
  int64_t nnodes;
  TG_TRY(tg_pp_setup("tg_quad_load", patch, 2, nullptr, &A, &lds, &nnodes));
  TG_REQUIRE(f_q && f_q->n == A.npts, "tg_quad_load: npts = %lld point values", (long long)A.npts);
  A.fq = f_q->d;
  TG_TRY(tg_point_nodal_output("tg_quad_load", out, nnodes, &A.out));
  return tg_pp_launch_rat<2>(rat, A, lds);
}

// ---- point coefficients.  The checks of the point arrays are shared: `n` values per point or null
static int tg_pp_point_array(const char *who, const char *name, tg_vec_t v, int64_t n, int64_t npts, const double **out) {
  *out = nullptr;
  if (!v) return 0;
  TG_REQUIRE(v->n == n * npts, "%s: %s holds %lld values, expected %lld per point of %lld points", who, name, (long long)v->n,
             (long long)n, (long long)npts);
  *out = v->d;
  return 0;
}

extern "C" int tg_coef_transform(const tg_patch_t *patch, int rational, int a_kind, tg_vec_t A_q, tg_vec_t b_q, tg_vec_t c_q,
                                 tg_vec_t m_q, tg_vec_t coef_out) {
  tg_pp_args A;
  size_t lds;
  TG_TRY(tg_pp_setup("tg_coef_transform", patch, 0, nullptr, &A, &lds));
  const int d = A.d, nsd = A.nsd;
  TG_REQUIRE(a_kind >= 0 && a_kind <= 2 && (a_kind == 0) == (A_q == nullptr),
             "tg_coef_transform: a_kind 0 = no diffusion (A_q null), 1 = one value per point, 2 = an nsd x nsd tensor per point");
  TG_REQUIRE(coef_out && coef_out->n == (int64_t)(d * d + 2 * d + 1) * A.npts,
             "tg_coef_transform: an output of (d^2 + 2 d + 1) npts = %lld values", (long long)((d * d + 2 * d + 1) * A.npts));
  A.akind = a_kind;
  TG_TRY(tg_pp_point_array("tg_coef_transform", "A_q", A_q, a_kind == 2 ? nsd * nsd : 1, A.npts, &A.Aq));
  TG_TRY(tg_pp_point_array("tg_coef_transform", "b_q", b_q, nsd, A.npts, &A.bq));
  TG_TRY(tg_pp_point_array("tg_coef_transform", "c_q", c_q, nsd, A.npts, &A.cq));
  TG_TRY(tg_pp_point_array("tg_coef_transform", "m_q", m_q, 1, A.npts, &A.mq));
  A.cout = coef_out->d;
  return tg_pp_launch_rat<TG_PP_COEF>(rational != 0, A, lds);
}

// the nF^2 blocks of a vector-valued unknown (nF = nsd = d fields on the scalar space): block (i, j) of A_q is the tensor
// A_ij[K][L] of d P_iK / d F_jL, block (i, j) of M_q the reaction of int v_i M_ij u_j; each block comes out as one scalar
// coefficient set of tg_coef_transform
extern "C" int tg_coef_transform_blocks(const tg_patch_t *patch, int rational, int nF, tg_vec_t A_q, tg_vec_t M_q, tg_vec_t coef_out) {
  tg_pp_args A;
  size_t lds;
  TG_TRY(tg_pp_setup("tg_coef_transform_blocks", patch, 0, nullptr, &A, &lds));
  const int d = A.d, nsd = A.nsd;
  TG_REQUIRE((d == 2 || d == 3) && nsd == d && nF == d,
             "tg_coef_transform_blocks: as many fields as physical and parametric directions, 2 or 3 (nF = %d, nsd = %d, d = %d)", nF,
             nsd, d);
  const int64_t nb = (int64_t)nF * nF;
  TG_REQUIRE(A_q, "tg_coef_transform_blocks: no tangent");
  TG_REQUIRE(coef_out && coef_out->n == nb * (d * d + 2 * d + 1) * A.npts,
             "tg_coef_transform_blocks: an output of nF^2 (d^2 + 2 d + 1) npts = %lld values",
             (long long)(nb * (d * d + 2 * d + 1) * A.npts));
  A.akind = 2;
  A.nblk = (int)nb;
  TG_TRY(tg_pp_point_array("tg_coef_transform_blocks", "A_q", A_q, nb * nsd * nsd, A.npts, &A.Aq));
  TG_TRY(tg_pp_point_array("tg_coef_transform_blocks", "M_q", M_q, nb, A.npts, &A.mq));
  A.cout = coef_out->d;
  return tg_pp_launch_rat<TG_PP_COEF | TG_PP_BLOCKS>(rational != 0, A, lds);
}

// a first-order system of nF fields on the scalar space (nF independent of nsd and d): block (i, j) with its own tensor, its
// vectors b_ij (pairs with grad v_i and u_j) and c_ij (pairs with v_i and grad u_j) and its reaction; any of the four null.
// The per-block body is the scalar ending's, so one field gives the bits of tg_coef_transform(a_kind = 2)
extern "C" int tg_coef_transform_system(const tg_patch_t *patch, int rational, int nF, tg_vec_t A_q, tg_vec_t b_q, tg_vec_t c_q,
                                        tg_vec_t M_q, tg_vec_t coef_out) {
  tg_pp_args A;
  size_t lds;
  TG_TRY(tg_pp_setup("tg_coef_transform_system", patch, 0, nullptr, &A, &lds));
  const int d = A.d, nsd = A.nsd;
  TG_REQUIRE(nF >= 1 && nF <= TG_SYSTEM_MAX_FIELDS, "tg_coef_transform_system: nF = %d; 1..%d fields", nF, TG_SYSTEM_MAX_FIELDS);
  const int64_t nb = (int64_t)nF * nF;
  TG_REQUIRE(coef_out && coef_out->n == nb * (d * d + 2 * d + 1) * A.npts,
             "tg_coef_transform_system: an output of nF^2 (d^2 + 2 d + 1) npts = %lld values",
             (long long)(nb * (d * d + 2 * d + 1) * A.npts));
  A.akind = A_q ? 2 : 0;
  A.nblk = (int)nb;
  TG_TRY(tg_pp_point_array("tg_coef_transform_system", "A_q", A_q, nb * nsd * nsd, A.npts, &A.Aq));
  TG_TRY(tg_pp_point_array("tg_coef_transform_system", "b_q", b_q, nb * nsd, A.npts, &A.bq));
  TG_TRY(tg_pp_point_array("tg_coef_transform_system", "c_q", c_q, nb * nsd, A.npts, &A.cq));
  TG_TRY(tg_pp_point_array("tg_coef_transform_system", "M_q", M_q, nb, A.npts, &A.mq));
  A.cout = coef_out->d;
  return tg_pp_launch_rat<TG_PP_COEF | TG_PP_BLOCKS>(rational != 0, A, lds);
}

// G = 4 P P^T at the points: nsd^2 npts values, component (K, L) at (K nsd + L) npts + q
extern "C" int tg_quad_metric(const tg_patch_t *patch, tg_vec_t G_out) {
  tg_pp_args A;
  size_t lds;
  TG_TRY(tg_pp_setup("tg_quad_metric", patch, 0, nullptr, &A, &lds));
  TG_REQUIRE(G_out && G_out->n == (int64_t)A.nsd * A.nsd * A.npts, "tg_quad_metric: an output of nsd^2 npts = %lld values",
             (long long)((int64_t)A.nsd * A.nsd * A.npts));
  A.cout = G_out->d;
  return tg_pp_launch<TG_PP_METRIC>(A, lds);
}

extern "C" int tg_flux_transform(const tg_patch_t *patch, int rational, tg_vec_t s_q, tg_vec_t F_q, tg_vec_t out) {
  tg_pp_args A;
  size_t lds;
  TG_TRY(tg_pp_setup("tg_flux_transform", patch, 0, nullptr, &A, &lds));
  TG_REQUIRE(out && out->n == (int64_t)(A.d + 1) * A.npts, "tg_flux_transform: an output of (d + 1) npts = %lld values",
             (long long)((A.d + 1) * A.npts));
  TG_TRY(tg_pp_point_array("tg_flux_transform", "s_q", s_q, 1, A.npts, &A.sq));
  TG_TRY(tg_pp_point_array("tg_flux_transform", "F_q", F_q, A.nsd, A.npts, &A.Fq));
  A.cout = out->d;
  return tg_pp_launch_rat<TG_PP_FLUX>(rational != 0, A, lds);
}

static int tg_pp_load_flux(const tg_patch_t *patch, tg_vec_t s_q, tg_vec_t F_q, tg_vec_t out, bool rat) {
  tg_pp_args A;
  size_t lds;
  int64_t nnodes;
  TG_TRY(tg_pp_setup("tg_quad_load_flux", patch, 4, nullptr, &A, &lds, &nnodes));
  TG_TRY(tg_pp_point_array("tg_quad_load_flux", "s_q", s_q, 1, A.npts, &A.sq));
  TG_TRY(tg_pp_point_array("tg_quad_load_flux", "F_q", F_q, A.nsd, A.npts, &A.Fq));
  TG_TRY(tg_point_nodal_output("tg_quad_load_flux", out, nnodes, &A.out));
  return tg_pp_launch_rat<2 | TG_PP_FLUX>(rat, A, lds);
}

static int tg_pp_error(const tg_patch_t *patch, tg_vec_t u_nodal, tg_vec_t e_q, tg_vec_t ge_q, double *out, bool rat) {
  tg_pp_args A;
  size_t lds;
  TG_REQUIRE(out, "tg_quad_error: no output");
  TG_TRY(tg_pp_setup("tg_quad_error", patch, 3, u_nodal, &A, &lds));
  TG_REQUIRE(!e_q || e_q->n == A.npts, "tg_quad_error: npts = %lld point values of e", (long long)A.npts);
  TG_REQUIRE(!ge_q || ge_q->n == (int64_t)A.nsd * A.npts, "tg_quad_error: nsd * npts = %lld point values of the gradient of e",
             (long long)(A.nsd * A.npts));
  A.eq = e_q ? e_q->d : nullptr;
  A.geq = ge_q ? ge_q->d : nullptr;
  tg_dbuf<double> part;
  TG_TRY(part.alloc(3 * A.nelem + 3));
  A.part = part.get();
  TG_TRY(tg_pp_launch_rat<3>(rat, A, lds));
  double *sums = part.get() + 3 * A.nelem;
  hipLaunchKernelGGL(k_postproc_fold, dim3(3), dim3(256), 0, g_tg.stream, part.get(), A.nelem, sums);
  TG_LAUNCH_CHECK();
  TG_CHECK_HIP(hipMemcpyAsync(g_tg.host_pinned, sums, 3 * sizeof(double), hipMemcpyDeviceToHost, g_tg.stream));
  TG_CHECK_HIP(hipStreamSynchronize(g_tg.stream));
  for (int t = 0; t < 3; t++) out[t] = g_tg.host_pinned[t];
  return 0;
}

extern "C" int tg_quad_eval(const tg_patch_t *patch, tg_vec_t u_nodal, int with_grad, tg_vec_t val_out, tg_vec_t grad_out) {
  return tg_pp_eval(patch, u_nodal, with_grad, val_out, grad_out, false);
}
extern "C" int tg_quad_load(const tg_patch_t *patch, tg_vec_t f_q, tg_vec_t out) { return tg_pp_load(patch, f_q, out, false); }
extern "C" int tg_quad_error(const tg_patch_t *patch, tg_vec_t u_nodal, tg_vec_t e_q, tg_vec_t ge_q, double *out) {
  return tg_pp_error(patch, u_nodal, e_q, ge_q, out, false);
}
// ---- rational functions u_h / W_h, tested against phi / W_h
extern "C" int tg_quad_eval_rational(const tg_patch_t *patch, tg_vec_t u_nodal, int with_grad, tg_vec_t val_out, tg_vec_t grad_out) {
  return tg_pp_eval(patch, u_nodal, with_grad, val_out, grad_out, true);
}
extern "C" int tg_quad_load_rational(const tg_patch_t *patch, tg_vec_t f_q, tg_vec_t out) { return tg_pp_load(patch, f_q, out, true); }
extern "C" int tg_quad_load_flux(const tg_patch_t *patch, tg_vec_t s_q, tg_vec_t F_q, tg_vec_t out) {
  return tg_pp_load_flux(patch, s_q, F_q, out, false);
}
extern "C" int tg_quad_load_flux_rational(const tg_patch_t *patch, tg_vec_t s_q, tg_vec_t F_q, tg_vec_t out) {
  return tg_pp_load_flux(patch, s_q, F_q, out, true);
}
extern "C" int tg_quad_error_rational(const tg_patch_t *patch, tg_vec_t u_nodal, tg_vec_t e_q, tg_vec_t ge_q, double *out) {
  return tg_pp_error(patch, u_nodal, e_q, ge_q, out, true);
}

// ---- lattice sampling: the points and the evaluation on m caller-given abscissae t[0..m) in [0, 1] per element and
// direction (the ends are allowed: the points on shared element faces then come once per element).  The kernel and its
// endings are those of the Gauss points; the table l | dl | w of this call is built here at the abscissae (the expressions
// of the Gauss table, tg_assemble.hip) and lives until the launch has run.  Numbering: tg_quad_points with m for nq.
static int tg_pp_lattice_setup(const char *who, const tg_patch_t *patch, int m, const double *t, tg_vec_t u, tg_pp_args *A, size_t *lds,
                               tg_dbuf<double> *tab) {
  TG_REQUIRE(patch, "%s: no patch", who);
  TG_REQUIRE(m >= 1 && m <= TG_ASM_MAXQ1 && t, "%s: m = %d; 1..%d abscissae per direction", who, m, TG_ASM_MAXQ1);
  for (int q = 0; q < m; q++)
    TG_REQUIRE(t[q] >= 0.0 && t[q] <= 1.0 && (q == 0 || t[q - 1] < t[q]), "%s: the abscissae increase within [0, 1] (t[%d] = %g)", who, q, t[q]);
  tg_patch_t pt = *patch;
  pt.nq = m;
  TG_TRY(tg_pp_setup(who, &pt, u ? 1 : 0, u, A, lds, nullptr, false));
  const int p = pt.p, p1 = p + 1;
  std::vector<double> h((size_t)2 * p1 * m + m, 1.0);      // (w = 1: the weights are not an output of these entries)
  for (int a = 0; a < p1; a++)
    for (int q = 0; q < m; q++) {
      double l = 1.0, dl = 0.0;
      for (int k = 0; k < p1; k++)
        if (k != a) l *= (t[q] - (double)k / p) / ((double)a / p - (double)k / p);
      for (int k = 0; k < p1; k++) {
        if (k == a) continue;
        double term = 1.0 / ((double)a / p - (double)k / p);
        for (int r = 0; r < p1; r++)
          if (r != a && r != k) term *= (t[q] - (double)r / p) / ((double)a / p - (double)r / p);
        dl += term;
      }
      h[(size_t)a * m + q] = l;
      h[(size_t)p1 * m + (size_t)a * m + q] = dl;
    }
  TG_TRY(tab->alloc((int64_t)h.size()));
  TG_TRY(tg_h2d_staged(tab->get(), h.data(), h.size() * sizeof(double)));
  A->tab = tab->get();
  return 0;
}

extern "C" int tg_lattice_points(const tg_patch_t *patch, int m, const double *t, tg_vec_t x_out) {
  tg_pp_args A;
  size_t lds;
  tg_dbuf<double> tab, wdet;
  TG_TRY(tg_pp_lattice_setup("tg_lattice_points", patch, m, t, nullptr, &A, &lds, &tab));
  TG_REQUIRE(x_out && x_out->n == (int64_t)A.nsd * A.npts, "tg_lattice_points: an output of nsd * npts = %lld values",
             (long long)(A.nsd * A.npts));
  TG_TRY(wdet.alloc(A.npts));      // (ending 0 writes sqrt(det g) next to the points; not handed out)
  A.x = x_out->d;
  A.wdet = wdet.get();
  return tg_pp_launch<0>(A, lds);
}

static int tg_pp_lattice_eval(const tg_patch_t *patch, int m, const double *t, tg_vec_t u_nodal, int with_grad, tg_vec_t val_out,
                              tg_vec_t grad_out, bool rat) {
  tg_pp_args A;
  size_t lds;
  tg_dbuf<double> tab;
  TG_REQUIRE(u_nodal, "tg_lattice_eval: no nodal vector");
  TG_TRY(tg_pp_lattice_setup("tg_lattice_eval", patch, m, t, u_nodal, &A, &lds, &tab));
  TG_REQUIRE(val_out && val_out->n == A.npts, "tg_lattice_eval: an output of npts = %lld values", (long long)A.npts);
  A.val = val_out->d;
  if (with_grad) {
    TG_REQUIRE(grad_out && grad_out->n == (int64_t)A.nsd * A.npts, "tg_lattice_eval: a gradient output of nsd * npts = %lld values",
               (long long)(A.nsd * A.npts));
    A.grad = grad_out->d;
  }
  return tg_pp_launch_rat<1>(rat, A, lds);
}

extern "C" int tg_lattice_eval(const tg_patch_t *patch, int m, const double *t, tg_vec_t u_nodal, int with_grad, tg_vec_t val_out,
                               tg_vec_t grad_out) {
  return tg_pp_lattice_eval(patch, m, t, u_nodal, with_grad, val_out, grad_out, false);
}
extern "C" int tg_lattice_eval_rational(const tg_patch_t *patch, int m, const double *t, tg_vec_t u_nodal, int with_grad,
                                        tg_vec_t val_out, tg_vec_t grad_out) {
  return tg_pp_lattice_eval(patch, m, t, u_nodal, with_grad, val_out, grad_out, true);
}
