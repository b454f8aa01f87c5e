// Boundary integrals on mapped tensor-product patches: the boundary measure and the mapped normal that the reference's
// ExtractedSpline offers next to dx (spline.ds = tIGArMeasure(surfaceJacobian(g, N), ds, ...), spline.n = mappedNormal(N, F),
// tIGAr/common.py:931-939; surfaceJacobian = sqrt(det g N.g^-1 N), mappedNormal = DF g^-1 N / |.|,
// tIGAr/calculusUtils.py:37-52, 71-80).
//
// Conventions of tg_postproc.hip: scalar Q_p Lagrange space on the tensor node grid, geometry F = cp[i]/cp[nsd],
// Gauss-Legendre with nq points per direction, everything in the coordinates of the reference element [0,1]^d, so that no
// element size appears.  A face is (direction k, side s), parametric normal N = (2s - 1) e_k; its face elements are the
// elements of the boundary layer seen from the face, lexicographic in the remaining directions with the lower direction
// fastest, the nq^(d-1) points of a face element likewise; arrays with several components are component-major.  d = 2, 3.
//
//   tg_face_points      x_q, wsurf_q = w_q sqrt(det g_hat (g_hat^-1)_kk), n = DF g^-1 N / |.|, h_n = 1 / sqrt((g_hat^-1)_kk)
//   tg_face_eval        u, the Cartesian gradient and d_n u = (g^-1 N).grad_xi u / sqrt(N.g^-1 N)
//   tg_face_load        out[node] += sum_q wsurf_q (f_q phi_node + fn_q d_n phi_node)
//   tg_face_matrix      A_ab = sum_q wsurf_q (a_q phi_a phi_b + b_q phi_a d_n phi_b + c_q d_n phi_a phi_b), own pattern
//   tg_face_matrix_add  the same entries times a factor into a matrix that holds them
//
// One kernel, four endings.  The NORMAL direction is contracted first: the FE nodes are equispaced with the end points
// included, so l_a(end) is a Kronecker delta -- a value on the face needs the node layer on the face only, a normal
// derivative one (p+1)-term contraction with dl_a(end) over the p + 1 layers of the boundary element.  The remaining d - 1
// directions go through LDS by sum factorisation as in k_postproc, the load goes back to the nodes the same way.  The
// matrix ending keeps the point coefficients in LDS and forms each entry of the face element's block from the 1-D tables.
// No floating-point atomics: load and matrix add face element by face element, colour by colour (parities of the
// tangential element indices, 2^(d-1) colours in ascending order).  Same inputs, same bits.
//
// RATIONAL functions psi = phi / W_h: u = u_h / W_h, grad_xi u = (grad_xi u_h - u grad_xi W_h) / W_h; a test function's
// value becomes phi / W_h and its grad_xi phi becomes (grad_xi phi - phi beta) / W_h, beta = grad_xi W_h / W_h.
//
// The check of the patch, the LDS fit, the colour loop and the nodal fields' has / ci are tg_point_shared.h's, shared with
// tg_postproc.hip and tg_coef.hip.
#include "tg_common.h"
#include "tg_point_shared.h"
#include <cmath>

struct tg_bd_args {
  int d, p, nsd, nq;
  int kdir, side;              // the face
  int dt, t[2];                // tangential directions, ascending (t[1] unused when dt == 1)
  int nel[3], n[3];            // elements / nodes per direction (1 beyond d)
  int nelt[2];                 // face elements per tangential direction (1 beyond dt)
  const double *f[5];          // nodal fields: 0..2 homogeneous coordinates (the first nsd), 3 the weight function, 4 u (or null)
  int nc;
  const double *tab;           // l[a][q] | dl[a][q] | w[q]
  double dle[TG_MAX_DEGREE + 1];   // dl_a at the face end of the normal direction
  int epg, szA, szB;           // face elements per workgroup, doubles per element of the two LDS areas
  int efirst[2], ncol[2], estep;   // the face elements of this launch
  int64_t nelem;               // ... their number
  int64_t npts;                // points of the face
  double *x, *wsurf, *normal, *hn;     // points (each may be null)
  double *val, *grad, *dn;             // eval (grad, dn may be null)
  const double *fq, *fnq;              // load (either may be null)
  double *out;
  const double *aq, *bq, *cq;          // matrix: point coefficients (each may be null)
  double scale;
  const int64_t *rowptr;
  const int32_t *col;
  double *mval;
};

// face element e of the launch -> element indices of the boundary-layer element; returns the face element's number
__device__ __forceinline__ int64_t tg_bd_element(const tg_bd_args &P, int64_t e, int *el) {
  const int e0 = P.efirst[0] + P.estep * (int)(e % P.ncol[0]);
  const int e1 = P.efirst[1] + P.estep * (int)(e / P.ncol[0]);
  el[0] = el[1] = el[2] = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (k == P.kdir) el[k] = P.side ? P.nel[k] - 1 : 0;
    if (k == P.t[0]) el[k] = e0;
    if (P.dt == 2 && k == P.t[1]) el[k] = e1;
  }
  return (int64_t)e0 + (int64_t)P.nelt[0] * e1;
}

// node (tangential local node at = b0 + (p+1) b1, layer m of the normal direction) of the element
__device__ __forceinline__ int64_t tg_bd_node(const tg_bd_args &P, const int *el, int at, int m) {
  const int p1 = P.p + 1;
  const int b0 = at % p1, b1 = at / p1;
  int64_t idx[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (k == P.kdir) idx[k] = el[k] * P.p + m;
    if (k == P.t[0]) idx[k] = el[k] * P.p + b0;
    if (P.dt == 2 && k == P.t[1]) idx[k] = el[k] * P.p + b1;
  }
  return idx[0] + (int64_t)P.n[0] * (idx[1] + (int64_t)P.n[1] * idx[2]);
}

// position of column c in the ascending row [lo, hi) of col, or -1
__device__ __forceinline__ int64_t tg_bd_find(const int32_t *col, int64_t lo, int64_t hi, int32_t c) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int32_t v = col[mid];
    if (v == c) return mid;
    if (v < c)
      lo = mid + 1;
    else
      hi = mid;
  }
  return -1;
}

// MODE 0 points, 1 eval, 2 load, 3 matrix; + 4 (TG_BD_RAT): rational functions (eval, load, matrix)
#define TG_BD_RAT 4
#define TG_BD_MATQ 7           // doubles per point of the matrix ending: three weights, cn[3], c.beta
template <int MODER>
__global__ void __launch_bounds__(256) k_boundary(tg_bd_args P) {
  constexpr int MODE = MODER & 3;
  constexpr bool RAT = (MODER & TG_BD_RAT) != 0;
  static_assert(!(RAT && MODE == 0), "the points do not depend on the function space");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int d = P.d, dt = P.dt, p1 = P.p + 1, nq = P.nq, nsd = P.nsd, nc = P.nc, epg = P.epg;
  const int kdir = P.kdir, t0 = P.t[0], t1 = dt == 2 ? P.t[1] : -1;
  const int mface = P.side ? P.p : 0;
  const int nlt = dt == 1 ? p1 : p1 * p1;          // tangential local nodes
  const int nqf = dt == 1 ? nq : nq * nq;          // points of a face element
  double *tl = reinterpret_cast<double *>(smem);   // l[a][q]
  double *tdl = tl + p1 * nq;                      // dl[a][q]
  double *tw = tdl + p1 * nq;                      // w[q]
  double *bufA = tw + nq;
  double *bufB = bufA + (size_t)epg * P.szA;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t g0 = (int64_t)blockIdx.x * epg;
  for (int s = tid; s < 2 * p1 * nq + nq; s += nt) tl[s] = P.tab[s];
  // ---- the normal direction first: area A [slot 0: the function on the face | slot 1: its normal derivative][field][node]
  for (int i = tid; i < epg * nlt; i += nt) {
    const int es = i / nlt, at = i - es * nlt;
    if (g0 + es >= P.nelem) continue;
    int el[3];
    tg_bd_element(P, g0 + es, el);
    double *A = bufA + (size_t)es * P.szA;
#pragma unroll
    for (int c = 0; c < 5; c++) {
      if (!tg_pt_has(c, nsd, P.f)) continue;
      double dn = 0.0, fv = 0.0;
      for (int m = 0; m < p1; m++) {
        const double v = P.f[c][tg_bd_node(P, el, at, m)];
        dn = fma(P.dle[m], v, dn);
        if (m == mface) fv = v;
      }
      const int ci = tg_pt_ci(c, nsd);
      A[ci * nlt + at] = fv;
      A[(nc + ci) * nlt + at] = dn;
    }
  }
  __syncthreads();
  // ---- 3-D: tangential direction t0 through LDS.  A [b0, b1] slots (F, Dn) -> B [q0, b1] slots (F, Dn, D0)
  if (dt == 2) {
    const int Sin = p1 * p1, Sout = nq * p1, work = nc * Sout;
    for (int i = tid; i < epg * work; i += nt) {
      const int es = i / work, r = i - es * work;
      if (g0 + es >= P.nelem) continue;
      const int ci = r / Sout, idx = r - ci * Sout;
      const int q0 = idx % nq, b1 = idx / nq;
      const double *I = bufA + (size_t)es * P.szA + ci * Sin + p1 * b1;
      double v0 = 0.0, v1 = 0.0, vd = 0.0;
      for (int a = 0; a < p1; a++) {
        const double l = tl[a * nq + q0], dl = tdl[a * nq + q0];
        const double f0 = I[a];
        v0 = fma(l, f0, v0);
        vd = fma(dl, f0, vd);
        v1 = fma(l, I[nc * Sin + a], v1);
      }
      double *O = bufB + (size_t)es * P.szB + ci * Sout;
      O[idx] = v0;
      O[nc * Sout + idx] = v1;
      O[2 * nc * Sout + idx] = vd;
    }
    __syncthreads();
  }
  // ---- the last tangential direction: a thread per point, results in registers
  const double *fin = dt == 2 ? bufB : bufA;
  double *oth = dt == 2 ? bufA : bufB;
  const int szf = dt == 2 ? P.szB : P.szA, szt = dt == 2 ? P.szA : P.szB;
  const int nqk = dt == 2 ? nq : 1;
  const int Sin = nqk * p1;
  const double sN = P.side ? 1.0 : -1.0;
  for (int i = tid; i < epg * nqf; i += nt) {
    const int es = i / nqf, q = i - es * nqf;
    if (g0 + es >= P.nelem) continue;
    const int Q = q % nqk, ql = q / nqk;
    double N[5], dN[5][3];
#pragma unroll
    for (int c = 0; c < 5; c++) {
      N[c] = 0.0;
      dN[c][0] = dN[c][1] = dN[c][2] = 0.0;
      if (!tg_pt_has(c, nsd, P.f)) continue;
      const double *I = fin + (size_t)es * szf + tg_pt_ci(c, nsd) * Sin;
      double v = 0.0, vn = 0.0, e0 = 0.0, vd = 0.0;
      for (int a = 0; a < p1; a++) {
        const double l = tl[a * nq + ql], dl = tdl[a * nq + ql];
        const int off = Q + nqk * a;
        const double f0 = I[off];
        v = fma(l, f0, v);
        vd = fma(dl, f0, vd);
        vn = fma(l, I[nc * Sin + off], vn);
        if (dt == 2) e0 = fma(l, I[2 * nc * Sin + off], e0);
      }
      N[c] = v;
#pragma unroll
      for (int m = 0; m < 3; m++) dN[c][m] = m == kdir ? vn : (m == t0 ? (dt == 2 ? e0 : vd) : (m == t1 ? vd : 0.0));
    }
    // DF[i][k] = d(N_i / W)/dxi_k ; metric g = DF^T DF  (the twin of quotient, DF and g: k_postproc, tg_postproc.hip)
    const double W = N[3];
    if constexpr (RAT && MODE == 1) {
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
      for (int m = 0; m < 3; m++) G[k][m] = DF[0][k] * DF[0][m] + DF[1][k] * DF[1][m] + DF[2][k] * DF[2][m];
    double gi[3][3];
    const double det = tg_point_metric_inverse<false>(d, G, gi);
    // g^-1 N, its length sqrt(N.g^-1 N) = sqrt((g^-1)_kk), and cn = g^-1 N / sqrt(N.g^-1 N): d_n = cn . grad_xi
    double gN[3];
#pragma unroll
    for (int m = 0; m < 3; m++) gN[m] = sN * (kdir == 0 ? gi[m][0] : (kdir == 1 ? gi[m][1] : gi[m][2]));
    const double gkk = fabs(kdir == 0 ? gi[0][0] : (kdir == 1 ? gi[1][1] : gi[2][2]));
    const double rs = 1.0 / sqrt(gkk);
    double cn[3];
#pragma unroll
    for (int m = 0; m < 3; m++) cn[m] = gN[m] * rs;
    const double wq = tw[q % nq] * (dt == 2 ? tw[q / nq] : 1.0);
    const double wsurf = wq * sqrt(fabs(det) * gkk);
    int el[3];
    const int64_t gp = tg_bd_element(P, g0 + es, el) * nqf + q;    // the point's number on the face
    if (MODE == 0) {
      if (P.x) {
#pragma unroll
        for (int c = 0; c < 3; c++)
          if (c < nsd) P.x[(int64_t)c * P.npts + gp] = N[c] / W;
      }
      if (P.wsurf) P.wsurf[gp] = wsurf;
      if (P.hn) P.hn[gp] = rs;
      if (P.normal) {
        double nr[3], s2 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          nr[c] = DF[c][0] * cn[0] + DF[c][1] * cn[1] + DF[c][2] * cn[2];
          s2 = fma(nr[c], nr[c], s2);
        }
        const double rn = 1.0 / sqrt(s2);
#pragma unroll
        for (int c = 0; c < 3; c++)
          if (c < nsd) P.normal[(int64_t)c * P.npts + gp] = nr[c] * rn;
      }
    } else if (MODE == 1) {
      P.val[gp] = N[4];
      if (P.dn) P.dn[gp] = cn[0] * dN[4][0] + cn[1] * dN[4][1] + cn[2] * dN[4][2];
      if (P.grad) {
        double t[3];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = gi[k][0] * dN[4][0] + gi[k][1] * dN[4][1] + gi[k][2] * dN[4][2];
#pragma unroll
        for (int c = 0; c < 3; c++)
          if (c < nsd) P.grad[(int64_t)c * P.npts + gp] = DF[c][0] * t[0] + DF[c][1] * t[1] + DF[c][2] * t[2];
      }
    } else {
      const double rw = RAT ? 1.0 / W : 1.0;
      const double cb = RAT ? (cn[0] * dN[3][0] + cn[1] * dN[3][1] + cn[2] * dN[3][2]) * rw : 0.0;   // cn . beta
      double *T = oth + (size_t)es * szt;
      if (MODE == 2) {
        // coefficients of phi, of d_t0 phi (d_t1 phi) and of d_k phi at this point
        const double f = P.fq ? P.fq[gp] : 0.0;
        if (P.fnq) {
          const double fn = P.fnq[gp], s = wsurf * rw * fn;
          T[q] = wsurf * rw * (f - fn * cb);
          T[nqf + q] = s * (t0 == 0 ? cn[0] : (t0 == 1 ? cn[1] : cn[2]));
          if (dt == 2) T[2 * nqf + q] = s * (t1 == 1 ? cn[1] : cn[2]);
          T[(dt + 1) * nqf + q] = s * (kdir == 0 ? cn[0] : (kdir == 1 ? cn[1] : cn[2]));
        } else {
          T[q] = wsurf * rw * f;
        }
      } else {
        const double s = wsurf * rw * rw;
        T[q] = P.aq ? s * P.aq[gp] : 0.0;
        T[nqf + q] = P.bq ? s * P.bq[gp] : 0.0;
        T[2 * nqf + q] = P.cq ? s * P.cq[gp] : 0.0;
        T[3 * nqf + q] = kdir == 0 ? cn[0] : (kdir == 1 ? cn[1] : cn[2]);
        T[4 * nqf + q] = t0 == 0 ? cn[0] : (t0 == 1 ? cn[1] : cn[2]);
        T[5 * nqf + q] = dt == 2 ? (t1 == 1 ? cn[1] : cn[2]) : 0.0;
        T[6 * nqf + q] = cb;
      }
    }
  }
  if (MODE == 0 || MODE == 1) return;
  __syncthreads();
  if (MODE == 3) {
    // ---- entries of the face element's block: (a, b) with a or b on the face layer; the others are structurally zero
    const int nloc = nlt * p1;                     // local node = at + nlt * layer
    const int nent = nloc * nloc;
    for (int i = tid; i < epg * nent; i += nt) {
      const int es = i / nent, r = i - es * nent;
      if (g0 + es >= P.nelem) continue;
      const int a = r / nloc, b = r - a * nloc;
      const int ata = a % nlt, ma = a / nlt, atb = b % nlt, mb = b / nlt;
      const bool fa = ma == mface, fb = mb == mface;
      if (!fa && !fb) continue;
      const int a0 = ata % p1, a1 = ata / p1, b0 = atb % p1, b1 = atb / p1;
      const double da = P.dle[ma], db = P.dle[mb];
      const double *T = oth + (size_t)es * szt;
      double acc = 0.0;
      for (int q = 0; q < nqf; q++) {
        const int q0 = q % nq, q1 = q / nq;        // (q1 = 0 when dt == 1)
        const double la0 = tl[a0 * nq + q0], lb0 = tl[b0 * nq + q0];
        const double la1 = dt == 2 ? tl[a1 * nq + q1] : 1.0, lb1 = dt == 2 ? tl[b1 * nq + q1] : 1.0;
        const double La = la0 * la1, Lb = lb0 * lb1;
        const double ck = T[3 * nqf + q], c0 = T[4 * nqf + q], c1 = T[5 * nqf + q], cb = T[6 * nqf + q];
        // d_n of the two functions (times W_h for the rational ones) and their values on the face
        double dna = ck * da * La, dnb = ck * db * Lb;
        if (fa) dna += c0 * tdl[a0 * nq + q0] * la1 + (dt == 2 ? c1 * la0 * tdl[a1 * nq + q1] : 0.0) - cb * La;
        if (fb) dnb += c0 * tdl[b0 * nq + q0] * lb1 + (dt == 2 ? c1 * lb0 * tdl[b1 * nq + q1] : 0.0) - cb * Lb;
        const double va = fa ? La : 0.0, vb = fb ? Lb : 0.0;
        acc = fma(T[q], va * vb, acc);
        acc = fma(T[nqf + q], va * dnb, acc);
        acc = fma(T[2 * nqf + q], dna * vb, acc);
      }
      int el[3];
      tg_bd_element(P, g0 + es, el);
      const int64_t row = tg_bd_node(P, el, ata, ma);
      const int64_t pos = tg_bd_find(P.col, P.rowptr[row], P.rowptr[row + 1], (int32_t)tg_bd_node(P, el, atb, mb));
      // face elements of one launch share no node (one colour): plain adds (the pattern was checked before the launch)
      if (pos >= 0) P.mval[pos] += P.scale * acc;
    }
    return;
  }
  // ---- load: the point coefficients back to the tangential nodes, direction by direction; channel 1 + j takes dl in
  // tangential direction j (the coefficient of d_tj phi), the others l.  Before direction k: [a_0 .. a_k-1 | q_k ..]
  const int nch = P.fnq ? dt + 2 : 1;
  double *cur = oth, *nxt = dt == 2 ? bufB : bufA;
  int szc = szt, szn = szf;
  int pk = 1, qrest = nqf / nq;
  for (int k = 0; k < dt; k++) {
    const int Sc = pk * nq * qrest, So = pk * p1 * qrest;
    for (int i = tid; i < epg * nch * So; i += nt) {
      const int es = i / (nch * So), r = i - es * nch * So;
      if (g0 + es >= P.nelem) continue;
      const int ch = r / So, idx = r - ch * So;
      const int Ai = idx % pk, t = idx / pk, ak = t % p1, R = t / p1;
      const double *I = cur + (size_t)es * szc + ch * Sc;
      const double *tb = ch == 1 + k ? tdl : tl;
      double acc = 0.0;
      for (int q = 0; q < nq; q++) acc = fma(tb[ak * nq + q], I[Ai + pk * (q + nq * R)], acc);
      nxt[(size_t)es * szn + ch * So + idx] = acc;
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
  // face elements of one launch share no node (one colour): plain adds, the colours follow each other in a fixed order
  const int nloc = nlt * p1;
  for (int i = tid; i < epg * nloc; i += nt) {
    const int es = i / nloc, a = i - es * nloc;
    if (g0 + es >= P.nelem) continue;
    const int at = a % nlt, m = a / nlt;
    if (nch == 1 && m != mface) continue;
    const double *R = cur + (size_t)es * szc;
    double v = 0.0;
    if (m == mface) {
      v = R[at];
      if (nch > 1) {
        v += R[nlt + at];
        if (dt == 2) v += R[2 * nlt + at];
      }
    }
    if (nch > 1) v = fma(P.dle[m], R[(dt + 1) * nlt + at], v);
    int el[3];
    tg_bd_element(P, g0 + es, el);
    P.out[tg_bd_node(P, el, at, m)] += v;
  }
}

// ---- the pattern of tg_face_matrix in closed form: the element coupling restricted to the boundary layer.  Per direction
// j a node t couples to the nodes [s_j(t), s_j(t) + c_j(t)): tangentially the elements it touches, normally the p + 1
// layers (no columns outside the layer: c = 0); the number of entries before row (i0, i1, i2) is a sum of products of the
// 1-D prefix counts P_j(t) = sum_{t' < t} c_j(t').
struct tg_bd_pat {
  int d, p, kdir, lo;          // lo: first node layer of the boundary element
  int n[3], nel[3];
};
__device__ __forceinline__ void tg_bd_span(const tg_bd_pat &S, int j, int t, int *start, int *count, int64_t *prefix) {
  const int p = S.p, p1 = p + 1;
  if (j >= S.d) {
    *start = 0;
    *count = 1;
    *prefix = t;
  } else if (j == S.kdir) {
    const bool in = t >= S.lo && t <= S.lo + p;
    *start = S.lo;
    *count = in ? p1 : 0;
    *prefix = (int64_t)p1 * min(max(t - S.lo, 0), p1);
  } else {
    const bool vertex = t % p == 0, inner = vertex && t > 0 && t < S.n[j] - 1;
    *start = vertex ? max(0, t - p) : (t / p) * p;
    *count = inner ? 2 * p + 1 : p1;
    *prefix = (int64_t)t * p1 + (int64_t)p * (t >= 1 ? min((t - 1) / p, S.nel[j] - 1) : 0);
  }
}
__global__ void __launch_bounds__(256) k_face_pattern(tg_bd_pat S, int64_t nnodes, int64_t *rowptr, int32_t *col) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nnodes) return;
  int64_t T[3];
  int s[3], c[3];
  int64_t P[3];
  for (int j = 0; j < 3; j++) tg_bd_span(S, j, S.n[j], &s[j], &c[j], &T[j]);      // totals per direction
  if (i == nnodes) {
    rowptr[i] = T[0] * T[1] * T[2];
    return;
  }
  const int i0 = (int)(i % S.n[0]), i1 = (int)((i / S.n[0]) % S.n[1]), i2 = (int)(i / ((int64_t)S.n[0] * S.n[1]));
  tg_bd_span(S, 0, i0, &s[0], &c[0], &P[0]);
  tg_bd_span(S, 1, i1, &s[1], &c[1], &P[1]);
  tg_bd_span(S, 2, i2, &s[2], &c[2], &P[2]);
  int64_t at = P[2] * T[1] * T[0] + (int64_t)c[2] * (P[1] * T[0] + (int64_t)c[1] * P[0]);
  rowptr[i] = at;
  if (c[0] == 0 || c[1] == 0 || c[2] == 0) return;
  for (int j2 = 0; j2 < c[2]; j2++)
    for (int j1 = 0; j1 < c[1]; j1++)
      for (int j0 = 0; j0 < c[0]; j0++)
        col[at++] = (int32_t)((s[0] + j0) + (int64_t)S.n[0] * ((s[1] + j1) + (int64_t)S.n[1] * (s[2] + j2)));
}

// does the matrix hold every entry the face writes?  *missing = 1 if not
__global__ void __launch_bounds__(256) k_face_pattern_check(tg_bd_args P, const int64_t *rowptr, const int32_t *col, int *missing) {
  const int p1 = P.p + 1;
  const int nlt = P.dt == 1 ? p1 : p1 * p1, nloc = nlt * p1;
  const int mface = P.side ? P.p : 0;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nent = (int64_t)nloc * nloc;
  if (i >= P.nelem * nent) return;
  const int64_t e = i / nent;
  const int r = (int)(i - e * nent), a = r / nloc, b = r - a * nloc;
  if (a / nlt != mface && b / nlt != mface) return;
  int el[3];
  tg_bd_element(P, e, el);
  const int64_t row = tg_bd_node(P, el, a % nlt, a / nlt);
  if (tg_bd_find(col, rowptr[row], rowptr[row + 1], (int32_t)tg_bd_node(P, el, b % nlt, b / nlt)) < 0) *missing = 1;
}

#define TG_BD_LDS_DEFAULT ((size_t)64 * 1024)

// checks patch and face, fills what every ending shares; `u`: the nodal vector taken to the points (may be null);
// `nch`: channels of the load ending
static int tg_bd_setup(const char *who, const tg_patch_t *pt, int dir, int side, int mode, int nch, tg_vec_t u, tg_bd_args *A,
                       size_t *lds, int64_t *nnodes_out) {
  tg_patch_dims D;
  TG_TRY(tg_patch_check(who, pt, 2, true, u, &D));
  TG_REQUIRE(dir >= 0 && dir < D.d && (side == 0 || side == 1), "%s: face (%d, %d): 0 <= direction < %d, side 0 or 1", who, dir,
             side, D.d);
  TG_REQUIRE(D.nnodes < (1ll << 31), "%s: too many FE nodes for 32-bit column indices", who);
  const int d = D.d, p = D.p, p1 = p + 1, nq = D.nq, dt = d - 1;
  tg_point_args_init(D, A);
  A->kdir = dir;
  A->side = side;
  A->dt = dt;
  A->t[0] = A->t[1] = -1;
  A->nelt[0] = A->nelt[1] = 1;
  for (int k = 0, j = 0; k < d; k++)
    if (k != dir) {
      A->t[j] = k;
      A->nelt[j] = A->nel[k];
      j++;
    }
  for (int j = 0; j < 2; j++) {
    A->efirst[j] = 0;
    A->ncol[j] = A->nelt[j];
  }
  A->estep = 1;
  A->nelem = (int64_t)A->nelt[0] * A->nelt[1];
  const int nlt = tg_ipow(p1, dt), nqf = tg_ipow(nq, dt);
  A->npts = A->nelem * nqf;
  A->nc = tg_point_fields(pt, u, A->f);
  // dl_a at the end of the reference interval: nodes a / p
  for (int a = 0; a < p1; a++) {
    const long double xe = side ? 1.0L : 0.0L;
    long double s = 0.0L;
    for (int m = 0; m < p1; m++) {
      if (m == a) continue;
      long double t = (long double)p / (long double)(a - m);
      for (int r = 0; r < p1; r++)
        if (r != a && r != m) t *= (xe * p - r) / (long double)(a - r);
      s += t;
    }
    A->dle[a] = (double)s;
  }
  TG_TRY(tg_asm_cache_get(pt));
  A->tab = g_asm_cache.tab;
  // LDS per face element.  Area A: the two slots after the normal contraction; 3-D: area B the three slots after
  // direction t0.  The area the last contraction does not read takes the point coefficients of load and matrix, and the
  // load goes back to the nodes through both.
  const int nc = A->nc;
  int szA = 2 * nc * nlt, szB = dt == 2 ? 3 * nc * nq * p1 : 0;
  int &other = dt == 2 ? szA : szB;
  if (mode == 2) {
    const int back = nch * tg_ipow(std::max(p1, nq), dt);
    szA = std::max(szA, back);
    szB = std::max(szB, back);
  }
  if (mode == 3) other = std::max(other, TG_BD_MATQ * nqf);
  A->szA = szA;
  A->szB = szB;
  // the matrix ending gives every face element a workgroup of its own: the (p+1)^2d entries of its block keep 256 threads
  // busy, and with several elements per workgroup the searches in the rows of the matrix, one after the other per
  // thread, set the time of the call whatever the size of the face
  tg_point_lds_fit(p1, nq, szA, szB, mode == 3 ? 1 : std::max(1, 256 / nqf), TG_BD_LDS_DEFAULT, &A->epg, lds);
  TG_REQUIRE(*lds <= TG_BD_LDS_DEFAULT, "%s: face element data (%zu B) does not fit in LDS", who, *lds);
  if (nnodes_out) *nnodes_out = D.nnodes;
  return 0;
}

template <int MODE>
static int tg_bd_launch(const tg_bd_args &A, size_t lds) {
  if (A.nelem <= 0) return 0;
  hipLaunchKernelGGL((k_boundary<MODE>), dim3((unsigned)tg_cdiv(A.nelem, A.epg)), dim3(256), lds, g_tg.stream, A);
  TG_LAUNCH_CHECK();
  return 0;
}

// the endings that add (MODE 2 into the nodes, 3 into the matrix) take one launch per colour of the tangential element
// indices, the others one launch; plain or rational
template <int M>
static int tg_bd_launch_rat(bool rat, tg_bd_args &A, size_t lds) {
  auto launch = [&] { return rat ? tg_bd_launch<M | TG_BD_RAT>(A, lds) : tg_bd_launch<M>(A, lds); };
  if (M < 2) return launch();
  A.estep = 2;
  return tg_for_colours(A.dt, A.nelt, [&](const int *efirst, const int *ncol, int64_t count) {
    std::copy_n(efirst, 2, A.efirst);
    std::copy_n(ncol, 2, A.ncol);
    A.nelem = count;
    return launch();
  });
}

extern "C" int tg_face_points(const tg_patch_t *patch, int dir, int side, tg_vec_t x_out, tg_vec_t wsurf_out, tg_vec_t normal_out,
                              tg_vec_t hn_out) {
  tg_bd_args A;
  size_t lds;
  TG_TRY(tg_bd_setup("tg_face_points", patch, dir, side, 0, 0, nullptr, &A, &lds, nullptr));
  TG_REQUIRE((!x_out || x_out->n == (int64_t)A.nsd * A.npts) && (!normal_out || normal_out->n == (int64_t)A.nsd * A.npts) &&
                 (!wsurf_out || wsurf_out->n == A.npts) && (!hn_out || hn_out->n == A.npts),
             "tg_face_points: outputs of nsd * npts = %lld (x, normal) and npts = %lld (wsurf, h_n) values",
             (long long)(A.nsd * A.npts), (long long)A.npts);
  A.x = x_out ? x_out->d : nullptr;
  A.wsurf = wsurf_out ? wsurf_out->d : nullptr;
  A.normal = normal_out ? normal_out->d : nullptr;
  A.hn = hn_out ? hn_out->d : nullptr;
  return tg_bd_launch<0>(A, lds);
}

static int tg_bd_eval(const tg_patch_t *patch, int dir, int side, tg_vec_t u_nodal, tg_vec_t val_out, tg_vec_t grad_out,
                      tg_vec_t dn_out, bool rat) {
  tg_bd_args A;
  size_t lds;
  TG_REQUIRE(u_nodal, "tg_face_eval: no nodal vector");
  TG_TRY(tg_bd_setup("tg_face_eval", patch, dir, side, 1, 0, u_nodal, &A, &lds, nullptr));
  TG_REQUIRE(val_out && val_out->n == A.npts && (!dn_out || dn_out->n == A.npts) &&
                 (!grad_out || grad_out->n == (int64_t)A.nsd * A.npts),
             "tg_face_eval: outputs of npts = %lld (values, d_n u) and nsd * npts = %lld (gradient) values", (long long)A.npts,
             (long long)(A.nsd * A.npts));
  A.val = val_out->d;
  A.grad = grad_out ? grad_out->d : nullptr;
  A.dn = dn_out ? dn_out->d : nullptr;
  return tg_bd_launch_rat<1>(rat, A, lds);
}

static int tg_bd_load(const tg_patch_t *patch, int dir, int side, tg_vec_t f_q, tg_vec_t fn_q, tg_vec_t out, bool rat) {
  tg_bd_args A;
  size_t lds;
  int64_t nnodes;
  const int dt = patch ? patch->d - 1 : 1;
  TG_TRY(tg_bd_setup("tg_face_load", patch, dir, side, 2, fn_q ? dt + 2 : 1, nullptr, &A, &lds, &nnodes));
  TG_REQUIRE((!f_q || f_q->n == A.npts) && (!fn_q || fn_q->n == A.npts) && out && out->n == nnodes,
             "tg_face_load: npts = %lld point values and an output on the %lld FE nodes", (long long)A.npts, (long long)nnodes);
  if (!f_q && !fn_q) return 0;
  A.fq = f_q ? f_q->d : nullptr;
  A.fnq = fn_q ? fn_q->d : nullptr;
  A.out = out->d;
  return tg_bd_launch_rat<2>(rat, A, lds);
}

// the entries of the face into (rowptr, col, val) of m, which must hold them; check: look first, error 3 if one is missing
static int tg_bd_matrix_into(const tg_patch_t *patch, int dir, int side, tg_vec_t a_q, tg_vec_t b_q, tg_vec_t c_q, double scale,
                             tg_csr_s *m, bool check, bool rat, const char *who) {
  tg_bd_args A;
  size_t lds;
  int64_t nnodes;
  TG_TRY(tg_bd_setup(who, patch, dir, side, 3, 0, nullptr, &A, &lds, &nnodes));
  TG_REQUIRE((!a_q || a_q->n == A.npts) && (!b_q || b_q->n == A.npts) && (!c_q || c_q->n == A.npts),
             "%s: npts = %lld point values per coefficient", who, (long long)A.npts);
  TG_REQUIRE(m && !m->rowcnt && !m->view && m->nrows == nnodes && m->ncols == nnodes,
             "%s: a canonical CSR matrix on the %lld FE nodes of the patch", who, (long long)nnodes);
  if (check) {
    int *flag = reinterpret_cast<int *>(g_tg.scratch);
    TG_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int), g_tg.stream));
    const int64_t nloc = tg_ipow(A.p + 1, A.d), work = A.nelem * nloc * nloc;
    TG_REQUIRE(tg_cdiv(work, 256) < (1ll << 31), "%s: too many face elements for one launch", who);
    hipLaunchKernelGGL(k_face_pattern_check, dim3((unsigned)tg_cdiv(work, 256)), dim3(256), 0, g_tg.stream, A, m->rowptr, m->col,
                       flag);
    TG_LAUNCH_CHECK();
    int *hflag = reinterpret_cast<int *>(g_tg.host_pinned);
    TG_CHECK_HIP(hipMemcpyAsync(hflag, flag, sizeof(int), hipMemcpyDeviceToHost, g_tg.stream));
    TG_CHECK_HIP(hipStreamSynchronize(g_tg.stream));
    if (*hflag) {
      tg_set_error("%s: the matrix lacks entries of the face (%d, %d); it is unchanged", who, dir, side);
      return 3;
    }
  }
  if (!a_q && !b_q && !c_q) return 0;
  // values change: what was recorded about the old ones is stale
  tg_dfree(m->diag_cache);
  m->diag_cache = nullptr;
  m->diag_rows = 0;
  m->sym_verified = 0;
  tg_sell_drop(m);
  if (m->sell_state > 0) m->sell_state = 0;
  A.aq = a_q ? a_q->d : nullptr;
  A.bq = b_q ? b_q->d : nullptr;
  A.cq = c_q ? c_q->d : nullptr;
  A.scale = scale;
  A.rowptr = m->rowptr;
  A.col = m->col;
  A.mval = m->val;
  return tg_bd_launch_rat<3>(rat, A, lds);
}

static int tg_bd_matrix(const tg_patch_t *patch, int dir, int side, tg_vec_t a_q, tg_vec_t b_q, tg_vec_t c_q, tg_csr_t *out,
                        bool rat) {
  tg_bd_args A;
  size_t lds;
  int64_t nnodes;
  TG_REQUIRE(out, "tg_face_matrix: no output");
  TG_TRY(tg_bd_setup("tg_face_matrix", patch, dir, side, 3, 0, nullptr, &A, &lds, &nnodes));
  tg_bd_pat S;
  S.d = A.d;
  S.p = A.p;
  S.kdir = dir;
  S.lo = side ? A.n[dir] - 1 - A.p : 0;
  int64_t nnz = 1;
  for (int k = 0; k < 3; k++) {
    S.n[k] = A.n[k];
    S.nel[k] = A.nel[k];
    if (k < A.d) nnz *= k == dir ? (int64_t)(A.p + 1) * (A.p + 1) : (int64_t)A.n[k] * (A.p + 1) + (int64_t)A.p * (A.nel[k] - 1);
  }
  tg_csr_s *m = nullptr;
  TG_TRY(tg_csr_alloc(nnodes, nnodes, nnz, &m));
  hipLaunchKernelGGL(k_face_pattern, dim3((unsigned)tg_cdiv(nnodes + 1, 256)), dim3(256), 0, g_tg.stream, S, nnodes, m->rowptr,
                     m->col);
  int rc = hipGetLastError() != hipSuccess;
  if (!rc) rc = hipMemsetAsync(m->val, 0, (size_t)nnz * sizeof(double), g_tg.stream) != hipSuccess;
  if (!rc) rc = tg_bd_matrix_into(patch, dir, side, a_q, b_q, c_q, 1.0, m, false, rat, "tg_face_matrix");
  if (rc) {
    tg_csr_destroy(m);
    return rc;
  }
  *out = m;
  return 0;
}

extern "C" int tg_face_eval(const tg_patch_t *patch, int dir, int side, tg_vec_t u_nodal, tg_vec_t val_out, tg_vec_t grad_out,
                            tg_vec_t dn_out) {
  return tg_bd_eval(patch, dir, side, u_nodal, val_out, grad_out, dn_out, false);
}
extern "C" int tg_face_load(const tg_patch_t *patch, int dir, int side, tg_vec_t f_q, tg_vec_t fn_q, tg_vec_t out) {
  return tg_bd_load(patch, dir, side, f_q, fn_q, out, false);
}
extern "C" int tg_face_matrix(const tg_patch_t *patch, int dir, int side, tg_vec_t a_q, tg_vec_t b_q, tg_vec_t c_q, tg_csr_t *out) {
  return tg_bd_matrix(patch, dir, side, a_q, b_q, c_q, out, false);
}
extern "C" int tg_face_matrix_add(const tg_patch_t *patch, int dir, int side, tg_vec_t a_q, tg_vec_t b_q, tg_vec_t c_q, double scale,
                                  tg_csr_t A) {
  return tg_bd_matrix_into(patch, dir, side, a_q, b_q, c_q, scale, A, true, false, "tg_face_matrix_add");
}
// ---- rational functions u_h / W_h, tested against phi / W_h
extern "C" int tg_face_eval_rational(const tg_patch_t *patch, int dir, int side, tg_vec_t u_nodal, tg_vec_t val_out,
                                     tg_vec_t grad_out, tg_vec_t dn_out) {
  return tg_bd_eval(patch, dir, side, u_nodal, val_out, grad_out, dn_out, true);
}
extern "C" int tg_face_load_rational(const tg_patch_t *patch, int dir, int side, tg_vec_t f_q, tg_vec_t fn_q, tg_vec_t out) {
  return tg_bd_load(patch, dir, side, f_q, fn_q, out, true);
}
extern "C" int tg_face_matrix_rational(const tg_patch_t *patch, int dir, int side, tg_vec_t a_q, tg_vec_t b_q, tg_vec_t c_q,
                                       tg_csr_t *out) {
  return tg_bd_matrix(patch, dir, side, a_q, b_q, c_q, out, true);
}
extern "C" int tg_face_matrix_add_rational(const tg_patch_t *patch, int dir, int side, tg_vec_t a_q, tg_vec_t b_q, tg_vec_t c_q,
                                           double scale, tg_csr_t A) {
  return tg_bd_matrix_into(patch, dir, side, a_q, b_q, c_q, scale, A, true, true, "tg_face_matrix_add_rational");
}
