// Volume forms with POINT COEFFICIENTS on mapped tensor-product patches: what a user of the reference writes as
// kappa*inner(spline.grad(u), spline.grad(v))*spline.dx, or gets from derivative(residual, u) of a quasilinear problem --
//
//   a(u, v) = int grad v . (A grad u) + (b . grad v) u + v (c . grad u) + m u v  dx      (u: trial = column, v: test = row)
//   L(v)    = int s v + F . grad v  dx
//
// with grad the Cartesian gradient DF g^-1 grad_xi, dx = sqrt(det g) dxi, and A (a scalar or an nsd x nsd tensor, not
// necessarily symmetric), b, c, F (nsd components), m, s given AT THE QUADRATURE POINTS, numbered as tg_quad_points,
// component-major.  Scalar Q_p space, d = 1, 2, 3, nsd >= d: the scope of tg_postproc.hip.
//
// Two steps.  (1) One pass over the points (an ending of k_postproc, tg_postproc.hip: the geometry is at the points there)
// brings the Cartesian data to the reference element [0,1]^d.  With P = DF g^-1 (nsd x d) and wdet = w sqrt(det g_hat):
//     C^ = wdet P^T A P    b^ = wdet P^T b    c^ = wdet P^T c    m^ = wdet m        s^ = wdet s    F^ = wdet P^T F
// (an isotropic A = a I gives C^ = wdet a g^-1, since P^T P = g^-1).  RATIONAL functions psi = phi / W_h fold into the same
// data: with beta = grad_xi W_h / W_h, grad_xi psi = (grad_xi phi - phi beta) / W_h, so that
//     C' = C^ / W^2                         b' = b^ / W^2 - C' beta            c' = c^ / W^2 - C'^T beta
//     m' = m^ / W^2 - beta . b^ / W^2 - beta . c^ / W^2 + beta . C' beta       F' = F^ / W      s' = (s^ - F^ . beta) / W
// and the element kernels need one variant and no control functions.  d^2 + 2d + 1 values per point for the matrix,
// d + 1 for the load.  (2) The element matrix from the transformed data,
//     A_e[a][b] = sum_q grad_xi phi_a . C_q grad_xi phi_b + (b_q . grad_xi phi_a) phi_b + phi_a (c_q . grad_xi phi_b) + m_q phi_a phi_b
// on the element-coupling pattern with its certificate.  3-D, nsd = 3, nq = p + 1, p = 2, 3 run sum-factorised: instantiations
// of k_asf3 / k_asf3_quad (tg_assemble.hip, TG_ASF_COEF) whose phase 0 is a load of the point data into the wave's LDS area.
// This file: the plain kernel for every d, p, nq, nsd that tg_assemble_limits allows (and for those shapes under
// TIGAR_ASM_LEGACY) -- one workgroup per element, the element's point data and the 1-D tables in LDS, one thread
// per pair (a, b).  Elements of one launch share no node (the colours of k_assemble_mapped, in the same order) and add
// without atomics: the same inputs give the same bits.  The load L(v) is an ending of k_postproc (tg_quad_load_flux).
#include "tg_common.h"
#include "tg_point_shared.h"

struct tg_coef_args {
  int d, p, nq;
  int nel[3], n[3];            // elements / nodes per direction (1 beyond d)
  const double *tab;           // l[a][q] | dl[a][q] | ...
  const double *coef;          // [d^2 + 2d + 1][npts]
  int64_t npts;
  const int64_t *rowptr;
  double *val;
  int efirst[3], ncol[3];      // this launch: the elements efirst[k] + 2 i, i < ncol[k]
};

__global__ void __launch_bounds__(256) k_coef_matrix(tg_coef_args P) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int d = P.d, p1 = P.p + 1, nq = P.nq;
  const int nloc = d == 1 ? p1 : (d == 2 ? p1 * p1 : p1 * p1 * p1);
  const int nqt = d == 1 ? nq : (d == 2 ? nq * nq : nq * nq * nq);
  const int ncomp = d * d + 2 * d + 1;
  double *tl = reinterpret_cast<double *>(smem);   // l[a][q]
  double *tdl = tl + p1 * nq;                      // dl[a][q]
  double *Cq = tdl + p1 * nq;                      // [ncomp][nqt]
  const int tid = threadIdx.x, nt = blockDim.x;
  int64_t e = blockIdx.x;
  int el[3] = {0, 0, 0};
  el[0] = 2 * (int)(e % P.ncol[0]) + P.efirst[0];
  e /= P.ncol[0];
  el[1] = 2 * (int)(e % P.ncol[1]) + P.efirst[1];
  e /= P.ncol[1];
  el[2] = 2 * (int)e + P.efirst[2];
  const int64_t q0 = ((int64_t)el[0] + (int64_t)P.nel[0] * ((int64_t)el[1] + (int64_t)P.nel[1] * el[2])) * nqt;   // first point
  for (int s = tid; s < 2 * p1 * nq; s += nt) tl[s] = P.tab[s];
  for (int s = tid; s < ncomp * nqt; s += nt) {
    const int c = s / nqt, q = s - c * nqt;
    Cq[s] = P.coef[(int64_t)c * P.npts + q0 + q];
  }
  __syncthreads();
  const double *Cb = Cq + d * d * nqt, *Cc = Cb + d * nqt, *Cm = Cc + d * nqt;
  for (int pr = tid; pr < nloc * nloc; pr += nt) {
    const int a = pr / nloc, b = pr - a * nloc;
    const int ak[3] = {a % p1, (a / p1) % p1, a / (p1 * p1)};
    const int bk[3] = {b % p1, (b / p1) % p1, b / (p1 * p1)};
    double acc = 0.0;
    for (int q = 0; q < nqt; q++) {
      const int qk[3] = {q % nq, (q / nq) % nq, q / (nq * nq)};
      // (constant indices after unrolling: the small arrays stay in registers)
      double la[3] = {1, 1, 1}, lb[3] = {1, 1, 1}, da[3] = {0, 0, 0}, db[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < 3; k++) {
        if (k >= d) continue;
        la[k] = tl[ak[k] * nq + qk[k]];
        lb[k] = tl[bk[k] * nq + qk[k]];
        da[k] = tdl[ak[k] * nq + qk[k]];
        db[k] = tdl[bk[k] * nq + qk[k]];
      }
      const double pa = la[0] * la[1] * la[2], pb = lb[0] * lb[1] * lb[2];
      const double ga[3] = {da[0] * la[1] * la[2], la[0] * da[1] * la[2], la[0] * la[1] * da[2]};
      const double gb[3] = {db[0] * lb[1] * lb[2], lb[0] * db[1] * lb[2], lb[0] * lb[1] * db[2]};
      // the column's flux X = C grad phi_b + b phi_b and value Xv = c . grad phi_b + m phi_b, then the row
      double t = Cm[q] * pb;
#pragma unroll
      for (int m = 0; m < 3; m++)
        if (m < d) t = fma(Cc[m * nqt + q], gb[m], t);
      t *= pa;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        if (k >= d) continue;
        double x = Cb[k * nqt + q] * pb;
#pragma unroll
        for (int m = 0; m < 3; m++)
          if (m < d) x = fma(Cq[(k * d + m) * nqt + q], gb[m], x);
        t = fma(ga[k], x, t);
      }
      acc += t;
    }
    // CSR slot of (row a, col b)
    int64_t row = 0, rstride = 1;
    int pos = 0, pstride = 1;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (k >= d) continue;
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

extern "C" int tg_assemble_coef_matrix(const tg_patch_t *pt, tg_vec_t coef, tg_csr_t *out) {
  tg_patch_dims D;
  TG_TRY(tg_patch_check("tg_assemble_coef_matrix", pt, 1, false, nullptr, &D));     // (the control functions are not read)
  TG_REQUIRE(out, "tg_assemble_coef_matrix: null output");
  const int d = D.d, p = D.p, p1 = p + 1, nq = D.nq, nqt = D.nqt;
  tg_coef_args A;
  memset(&A, 0, sizeof(A));
  A.d = d;
  A.p = p;
  A.nq = nq;
  for (int k = 0; k < 3; k++) {
    A.nel[k] = D.nel[k];
    A.n[k] = D.n[k];
  }
  const int ncomp = d * d + 2 * d + 1;
  A.npts = D.npts;
  TG_REQUIRE(coef && coef->n == (int64_t)ncomp * A.npts,
             "tg_assemble_coef_matrix: (d^2 + 2 d + 1) npts = %lld transformed point coefficients (tg_coef_transform)",
             (long long)(ncomp * A.npts));
  A.coef = coef->d;
  bool taken = false;                  // 3-D, nq = p + 1, p = 2, 3: sum-factorised (tg_assemble.hip)
  TG_TRY(tg_asm_coef_fast(pt, coef, out, &taken));
  if (taken) return 0;
  TG_TRY(tg_asm_cache_get(pt));
  A.tab = g_asm_cache.tab;
  // the element's point data in LDS: up to 16 x 1000 doubles (3-D, nq = 10), more than a launch gets without asking
  const size_t lds = ((size_t)2 * p1 * nq + (size_t)ncomp * nqt) * sizeof(double);
  TG_REQUIRE(lds <= (size_t)160 * 1024, "element data (%zu B) does not fit in LDS", lds);
  if (lds > (size_t)64 * 1024)
    TG_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_coef_matrix), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     160 * 1024));
  tg_csr_t m = nullptr;
  TG_TRY(tg_asm_coupling_pattern(d, p, A.n, 0, D.nnodes, false, &m));    // (values 0: the colours add into them)
  A.rowptr = m->rowptr;
  A.val = m->val;
  const bool timeit = getenv("TIGAR_ASM_TIME") != nullptr;
  if (timeit) hipEventRecord(g_tg.ev0[0], g_tg.stream);
  const int rc = tg_for_colours(d, A.nel, [&](const int *efirst, const int *ncol, int64_t nblk) {
    if (nblk >= (1ll << 31)) return 2;
    std::copy_n(efirst, 3, A.efirst);
    std::copy_n(ncol, 3, A.ncol);
    hipLaunchKernelGGL(k_coef_matrix, dim3((unsigned)nblk), dim3(256), lds, g_tg.stream, A);
    return hipGetLastError() != hipSuccess ? 1 : 0;
  });
  if (rc == 2) {
    tg_csr_destroy(m);
    tg_set_error("too many elements for one launch");
    return 2;
  }
  if (timeit) {
    hipEventRecord(g_tg.ev1[0], g_tg.stream);
    hipEventSynchronize(g_tg.ev1[0]);
    float ms = 0.f;
    hipEventElapsedTime(&ms, g_tg.ev0[0], g_tg.ev1[0]);
    fprintf(stderr, "[tg_assemble] coefficient form, %lld points: element kernels %.3f ms (plain)\n", (long long)A.npts, ms);
  }
  if (rc) {
    tg_csr_destroy(m);
    tg_set_error("the coefficient-form kernel failed to launch");
    return 1;
  }
  *out = m;
  return 0;
}

// ---- vector-valued unknowns: nF = d fields on the scalar space, dofs field after field (the space of the elasticity form).
// `coef_blocks`: nF^2 consecutive coefficient sets (tg_coef_transform_blocks), block (i, j) = test field i, trial field j.
// Every block goes through the driver above on a VIEW of its slice (no copy of the point data; the routes, TIGAR_ASM_LEGACY,
// TIGAR_ASM_CHUNK and TIGAR_ASM_QUAD_CHUNK as for one scalar form), a block row at a time, and the nF n square matrix is
// put together by tg_csr_from_blocks -- as the matrix of the mapped elasticity form is.
static int tg_coef_blocks_assemble(const tg_patch_t *pt, int nF, tg_vec_t coef_blocks, tg_csr_t *out) {
  const int64_t each = coef_blocks->n / ((int64_t)nF * nF);
  tg_csr_t blocks[TG_SYSTEM_MAX_FIELDS * TG_SYSTEM_MAX_FIELDS] = {nullptr};
  int rc = 0;
  for (int b = 0; b < nF * nF && !rc; b++) {
    tg_vec_s view;                     // (tg_assemble_coef_matrix checks its length against the patch)
    view.n = each;
    view.d = coef_blocks->d + (int64_t)b * each;
    rc = tg_assemble_coef_matrix(pt, &view, &blocks[b]);
  }
  if (!rc && nF == 1) {                // (one field: the block itself)
    *out = blocks[0];
    return 0;
  }
  if (!rc) rc = tg_csr_from_blocks(nF, blocks, out);
  for (int b = 0; b < nF * nF; b++)
    if (blocks[b]) tg_csr_destroy(blocks[b]);
  return rc;
}

extern "C" int tg_assemble_coef_blocks(const tg_patch_t *pt, int nF, tg_vec_t coef_blocks, tg_csr_t *out) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(pt && out && (pt->d == 2 || pt->d == 3) && nF == pt->d && pt->nsd == pt->d,
             "tg_assemble_coef_blocks: as many fields as physical and parametric directions, 2 or 3");
  TG_REQUIRE(coef_blocks && coef_blocks->n > 0 && coef_blocks->n % ((int64_t)nF * nF) == 0,
             "tg_assemble_coef_blocks: nF^2 = %d coefficient sets of equal length (tg_coef_transform_blocks)", nF * nF);
  return tg_coef_blocks_assemble(pt, nF, coef_blocks, out);
}

// ... of a first-order system (tg_coef_transform_system): any 1 <= nF <= TG_SYSTEM_MAX_FIELDS fields, d = 1, 2, 3, nsd >= d
extern "C" int tg_assemble_coef_system(const tg_patch_t *pt, int nF, tg_vec_t coef_blocks, tg_csr_t *out) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(pt && out && nF >= 1 && nF <= TG_SYSTEM_MAX_FIELDS, "tg_assemble_coef_system: a patch, an output and 1..%d fields",
             TG_SYSTEM_MAX_FIELDS);
  TG_REQUIRE(coef_blocks && coef_blocks->n > 0 && coef_blocks->n % ((int64_t)nF * nF) == 0,
             "tg_assemble_coef_system: nF^2 = %d coefficient sets of equal length (tg_coef_transform_system)", nF * nF);
  return tg_coef_blocks_assemble(pt, nF, coef_blocks, out);
}
