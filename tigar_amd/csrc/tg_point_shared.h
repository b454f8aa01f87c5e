// What the point kernels on mapped patches share (tg_postproc.hip: the volume; tg_boundary.hip: the faces; tg_coef.hip: the
// plain point-coefficient matrix; tg_assemble.hip: the host driver of the mapped forms, host side only): ONE check of the patch description, the LDS fit, the loop over the colours, the zeroed
// nodal output; on the device which nodal fields are present and where, and the inverse of a point's metric.  All static
// inline or templates: a host build has tg_postproc.hip and tg_coef.hip in one translation unit (tools/host_shim).
// NOT shared: the contractions through LDS to the points and back (slot layouts, merged slots and channels differ), and the
// quotient rule with DF and g = DF^T DF, twins in k_postproc and k_boundary: in a shared function they cost k_postproc
// registers and a wave of occupancy (profiles/point_kernels_refactor.md).
#pragma once
#include "tg_asm_shared.h"
#include <algorithm>

struct tg_patch_dims {
  int d, p, nsd, nq, nloc, nqt;      // nloc = (p+1)^d local nodes, nqt = nq^d points of an element
  int nel[3], n[3];                  // elements / FE nodes per direction (1 beyond d)
  int64_t nnodes, nelem, npts;
};

static inline int tg_ipow(int b, int e) {
  int r = 1;
  for (int i = 0; i < e; i++) r *= b;
  return r;
}

// the patch description of a point kernel: dmin <= d <= 3 (1 the volume entries, 2 the faces); `fields`: the nsd + 1 control
// functions are read and must lie on the FE nodes, as must `u`, the nodal vector taken to the points (may be null)
static inline int tg_patch_check(const char *who, const tg_patch_t *pt, int dmin, bool fields, tg_vec_t u, tg_patch_dims *D) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(pt && pt->d >= dmin && pt->d <= 3 && pt->p >= 1 && pt->p <= TG_MAX_DEGREE && pt->nsd >= pt->d && pt->nsd <= 3,
             "%s: a patch with %d <= d <= 3, d <= nsd <= 3 and 1 <= p <= %d", who, dmin, TG_MAX_DEGREE);
  TG_REQUIRE(pt->nq >= 1 && pt->nq <= TG_ASM_MAXQ1, "%s: 1..%d Gauss points per direction", who, TG_ASM_MAXQ1);
  D->d = pt->d;
  D->p = pt->p;
  D->nsd = pt->nsd;
  D->nq = pt->nq;
  D->nloc = tg_ipow(pt->p + 1, pt->d);
  D->nqt = tg_ipow(pt->nq, pt->d);
  TG_REQUIRE(D->nloc <= TG_ASM_MAXLOC, "%s: (p+1)^d = %d local nodes exceed the kernel limit %d", who, D->nloc, TG_ASM_MAXLOC);
  D->nnodes = D->nelem = 1;
  for (int k = 0; k < 3; k++) D->nel[k] = D->n[k] = 1;
  for (int k = 0; k < D->d; k++) {
    TG_REQUIRE(pt->nverts[k] >= 2 && pt->verts[k], "%s: direction %d needs at least one element", who, k);
    D->nel[k] = pt->nverts[k] - 1;
    D->n[k] = D->nel[k] * D->p + 1;
    D->nnodes *= D->n[k];
    D->nelem *= D->nel[k];
  }
  D->npts = D->nelem * D->nqt;
  for (int c = 0; fields && c <= D->nsd; c++)
    TG_REQUIRE(pt->cp[c] && pt->cp[c]->n == D->nnodes, "%s: control function %d: a vector on the %lld FE nodes of the patch", who, c,
               (long long)D->nnodes);
  TG_REQUIRE(!u || u->n == D->nnodes, "%s: the nodal vector holds %lld values, the patch has %lld FE nodes", who,
             (long long)(u ? u->n : 0), (long long)D->nnodes);
  return 0;
}

// zeroes the arguments of k_postproc / k_boundary / k_assemble_mapped and fills what all have from the patch
template <class Args>
static inline void tg_point_args_init(const tg_patch_dims &D, Args *A) {
  memset(A, 0, sizeof(*A));
  A->d = D.d, A->p = D.p, A->nsd = D.nsd, A->nq = D.nq;
  for (int k = 0; k < 3; k++) A->nel[k] = D.nel[k], A->n[k] = D.n[k];
}

// the nodal fields of the point kernels' arguments: 0..2 the homogeneous coordinates (the first nsd), 3 the weight function,
// 4 u (or null); returns how many there are
static inline int tg_point_fields(const tg_patch_t *pt, tg_vec_t u, const double **f) {
  for (int c = 0; c <= pt->nsd; c++) f[c < pt->nsd ? c : 3] = pt->cp[c]->d;
  if (u) f[4] = u->d;
  return pt->nsd + 1 + (u ? 1 : 0);
}

// elements per workgroup, from epg_start down, until the tables and the two LDS areas (szA, szB doubles per element) fit in
// `limit` bytes -- or one element is left, which may need more: *bytes says what the launch asks for
static inline void tg_point_lds_fit(int p1, int nq, int szA, int szB, int epg_start, size_t limit, int *epg, size_t *bytes) {
  auto need = [&](int e) { return ((size_t)2 * p1 * nq + nq + (size_t)e * ((size_t)szA + szB)) * sizeof(double); };
  *epg = epg_start;
  while (*epg > 1 && need(*epg) > limit) (*epg)--;
  *bytes = need(*epg);
}

// one launch per colour: the elements efirst[k] + 2 i, i < ncol[k], of [lo[k], hi[k]) with the parities of the element
// indices in the first ndir directions (0 and 1 beyond), colours in ascending order, empty ones skipped.  A direction whose
// bit is set in `uncoloured` is one colour: efirst = lo, ncol as for parity 0 but not a factor of count (the launch walks along
// it, or counts it its own way).  launch(efirst, ncol, count) returns 0 to go on
template <class F>
static inline int tg_for_colours(int ndir, const int *lo, const int *hi, unsigned uncoloured, F &&launch) {
  for (int c = 0; c < (1 << ndir); c++) {
    if (c & uncoloured) continue;
    int efirst[3] = {0, 0, 0}, ncol[3] = {1, 1, 1};
    int64_t count = 1;
    for (int k = 0; k < ndir; k++) {
      const bool coloured = !((uncoloured >> k) & 1);
      efirst[k] = coloured ? lo[k] + ((lo[k] ^ (c >> k)) & 1) : lo[k];       // the first index >= lo of this parity
      ncol[k] = hi[k] > efirst[k] ? (hi[k] - efirst[k] + 1) / 2 : 0;
      if (coloured) count *= ncol[k];
    }
    if (count == 0) continue;
    TG_TRY(launch(efirst, ncol, count));
  }
  return 0;
}

// ... every element of every direction, all directions coloured
template <class F>
static inline int tg_for_colours(int ndir, const int *nel, F &&launch) {
  const int lo[3] = {0, 0, 0};
  return tg_for_colours(ndir, lo, nel, 0u, launch);
}

// an output on the FE nodes, zeroed: the colours add into it
static inline int tg_point_nodal_output(const char *who, tg_vec_t out, int64_t nnodes, double **p) {
  TG_REQUIRE(out && out->n == nnodes, "%s: an output on the %lld FE nodes", who, (long long)nnodes);
  TG_CHECK_HIP(hipMemsetAsync(out->d, 0, (size_t)nnodes * sizeof(double), g_tg.stream));
  *p = out->d;
  return 0;
}

// is nodal field c there, and its position among the fields present
__device__ __forceinline__ bool tg_pt_has(int c, int nsd, const double *const *f) { return c < 3 ? c < nsd : f[c] != nullptr; }
__device__ __forceinline__ int tg_pt_ci(int c, int nsd) { return c < 3 ? c : nsd + (c - 3); }

// inverse gi (zero beyond) and determinant of the leading d x d block of a point's metric G = DF^T DF.  D1: d == 1 occurs
// (k_postproc; not on a face).  gi is zeroed HERE and the arrays have constant indices in every branch: they stay in registers
template <bool D1>
__device__ __forceinline__ double tg_point_metric_inverse(int d, const double (*G)[3], double (*gi)[3]) {
  double det;
#pragma unroll
  for (int k = 0; k < 3; k++) gi[k][0] = gi[k][1] = gi[k][2] = 0.0;
  double gm[9], gq[9];
  if (D1 && d == 1) {
    gm[0] = G[0][0];
    tg_sym_inverse(1, gm, gq, &det);
    gi[0][0] = gq[0];
  } else if (d == 2) {
    gm[0] = G[0][0];
    gm[1] = G[0][1];
    gm[2] = G[1][0];
    gm[3] = G[1][1];
    tg_sym_inverse(2, gm, gq, &det);
    gi[0][0] = gq[0];
    gi[0][1] = gq[1];
    gi[1][0] = gq[2];
    gi[1][1] = gq[3];
  } else {
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int m = 0; m < 3; m++) gm[3 * k + m] = G[k][m];
    tg_sym_inverse(3, gm, gq, &det);
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int m = 0; m < 3; m++) gi[k][m] = gq[3 * k + m];
  }
  return det;
}
