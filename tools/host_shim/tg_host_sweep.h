// What the sanitizer sweeps of the point kernels share (tools/coef_host_sweep.cpp, tools/material_host_sweep.cpp): the kernel
// source of csrc/tg_postproc.hip and csrc/tg_coef.hip WITH their host drivers, compiled as plain C++ against this directory's
// hip/hip_runtime.h, and host stand-ins for what those drivers call in the rest of the library -- the allocator, the
// reference-element tables, the element-coupling pattern, tg_csr_from_blocks -- each allocating EXACTLY what the kernels may
// touch.  Both sources include csrc/tg_point_shared.h (static inline and templates only: one translation unit here).  Include
// once, from the file that has main().  TG_HOST_SWEEP_JET (tools/jet_host_sweep.cpp, tools/shell_hyper_host_sweep.cpp): also
// csrc/tg_jet.hip and csrc/tg_shell.hip,
// whose kernels read the fourth table d2l[a][q] and the device copies of the element vertices: both are then allocated, again
// at exactly their sizes.  TG_HOST_SWEEP_SAMPLE (tools/sample_host_sweep.cpp): also csrc/tg_sample.hip, whose kernels stride
// over a capped grid (gridDim) and keep their own copies of the vertices.
#pragma once
#include <hip/hip_runtime.h>
dim3 threadIdx, blockIdx, blockDim, gridDim;
__attribute__((aligned(16))) char smem[TG_HOST_LDS_BYTES];
size_t g_host_lds_max = 0;

#include "../../tigar_amd/csrc/tg_postproc.hip"
#include "../../tigar_amd/csrc/tg_coef.hip"
#ifdef TG_HOST_SWEEP_JET
#include "../../tigar_amd/csrc/tg_jet.hip"
#include "../../tigar_amd/csrc/tg_shell.hip"
#endif
#ifdef TG_HOST_SWEEP_SAMPLE
#include "../../tigar_amd/csrc/tg_sample.hip"
#endif
#include <cstdarg>
#include <random>

tg_ctx_t g_tg;
tg_asm_cache_t g_asm_cache;
static char g_err[1024];
void tg_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int tg_dmalloc_bytes(void **p, size_t bytes) {
  *p = malloc(bytes);
  return *p ? 0 : 1;
}
void tg_dfree(void *p) { free(p); }
int tg_h2d_staged(void *dst, const void *src, size_t bytes) {   // (the lattice table of tg_postproc.hip, the vertices of tg_sample.hip)
  memcpy(dst, src, bytes);
  return 0;
}
extern "C" int tg_csr_destroy(tg_csr_t m) {
  if (m) {
    free(m->rowptr);
    free(m->val);
    delete m;
  }
  return 0;
}
int tg_asm_coef_fast(const tg_patch_t *, tg_vec_t, tg_csr_t *, bool *taken) {
  *taken = false;
  return 0;
}

// l[a][q] | dl[a][q] | w[q] on [0, 1] (values to rounding only: this program checks addresses, not figures)
int tg_asm_cache_get(const tg_patch_t *pt) {
  const int p = pt->p, p1 = p + 1, nq = pt->nq;
  free(g_asm_cache.tab);
#ifdef TG_HOST_SWEEP_JET
  double *tab = (double *)malloc(((size_t)3 * p1 * nq + nq) * sizeof(double));      // (l | dl | w | d2l: exactly what the kernels may read)
  for (int k = 0; k < 3; k++) {
    free(g_asm_cache.verts[k]);
    g_asm_cache.verts[k] = nullptr;
    if (k >= pt->d) continue;
    g_asm_cache.verts[k] = (double *)malloc(pt->nverts[k] * sizeof(double));
    memcpy(g_asm_cache.verts[k], pt->verts[k], pt->nverts[k] * sizeof(double));
  }
#else
  double *tab = (double *)malloc(((size_t)2 * p1 * nq + nq) * sizeof(double));      // (exactly what the kernels may read)
#endif
  for (int q = 0; q < nq; q++) {
    double z = cos(M_PI * (q + 0.75) / (nq + 0.5)), pp = 1.0;
    for (int it = 0; it < 50; it++) {
      double a = 1.0, b = 0.0;
      for (int j = 0; j < nq; j++) {
        const double c = b;
        b = a;
        a = ((2.0 * j + 1.0) * z * b - j * c) / (j + 1.0);
      }
      pp = nq * (z * a - b) / (z * z - 1.0);
      z -= a / pp;
    }
    const double t = 0.5 * (z + 1.0);
    tab[2 * p1 * nq + q] = 1.0 / ((1.0 - z * z) * pp * pp);
    for (int a = 0; a < p1; a++) {
      double l = 1.0, dl = 0.0;
      for (int m = 0; m < p1; m++)
        if (m != a) l *= (t - (double)m / p) / ((double)(a - m) / p);
      for (int m = 0; m < p1; m++) {
        if (m == a) continue;
        double term = 1.0 / ((double)(a - m) / p);
        for (int r = 0; r < p1; r++)
          if (r != a && r != m) term *= (t - (double)r / p) / ((double)(a - r) / p);
        dl += term;
      }
      tab[a * nq + q] = l;
      tab[p1 * nq + a * nq + q] = dl;
#ifdef TG_HOST_SWEEP_JET
      double d2l = 0.0;
      for (int m = 0; m < p1; m++)
        for (int r = 0; r < p1; r++) {
          if (m == a || r == a || r == m) continue;
          double term = 1.0 / (((double)(a - m) / p) * ((double)(a - r) / p));
          for (int u = 0; u < p1; u++)
            if (u != a && u != m && u != r) term *= (t - (double)u / p) / ((double)(a - u) / p);
          d2l += term;
        }
      tab[2 * p1 * nq + nq + a * nq + q] = d2l;
#endif
    }
  }
  g_asm_cache.tab = tab;
  return 0;
}

int tg_asm_coupling_pattern(int d, int p, const int *n, int64_t row0, int64_t row1, bool, tg_csr_t *out) {
  int64_t nrows = 1;
  for (int k = 0; k < d; k++) nrows *= n[k];
  if (row0 != 0 || row1 != nrows) return 2;
  tg_csr_s *m = new tg_csr_s;
  m->nrows = m->ncols = nrows;
  m->rowptr = (int64_t *)malloc((nrows + 1) * sizeof(int64_t));
  int64_t nnz = 0;
  for (int64_t r = 0; r < nrows; r++) {
    m->rowptr[r] = nnz;
    int64_t w = 1, rr = r;
    for (int k = 0; k < d; k++) {
      const int rk = (int)(rr % n[k]);
      rr /= n[k];
      w *= rk % p == 0 ? std::min(n[k] - 1, rk + p) - std::max(0, rk - p) + 1 : p + 1;
    }
    nnz += w;
  }
  m->rowptr[nrows] = nnz;
  m->nnz = nnz;
  m->val = (double *)calloc(nnz, sizeof(double));                                   // exactly nnz: no padding
  *out = m;
  return 0;
}

static std::mt19937_64 g_rng(12345);
static tg_vec_s *vec(int64_t n, double lo, double hi) {
  tg_vec_s *v = new tg_vec_s;
  v->n = n;
  v->d = (double *)malloc(std::max<int64_t>(n, 1) * sizeof(double));
  std::uniform_real_distribution<double> u(lo, hi);
  for (int64_t i = 0; i < n; i++) v->d[i] = u(g_rng);
  return v;
}
static void drop(tg_vec_s *v) {
  if (v) free(v->d);
  delete v;
}
#define CHECK(call)                                                      \
  do {                                                                   \
    if ((call) != 0) {                                                   \
      fprintf(stderr, "%s failed: %s\n", #call, g_err);                  \
      return 1;                                                          \
    }                                                                    \
  } while (0)

// every output array passes through here: finite, and folded into a running 64-bit FNV-1a of its bytes.  Two builds of a
// sweep (without sanitizers, -ffp-contract=off) that print the same value computed the same numbers
static uint64_t g_fnv = 1469598103934665603ull;
static int finite_all(const double *v, int64_t n) {
  const unsigned char *b = reinterpret_cast<const unsigned char *>(v);
  for (int64_t i = 0; i < n * (int64_t)sizeof(double); i++) g_fnv = (g_fnv ^ b[i]) * 1099511628211ull;
  for (int64_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return 0;
  return 1;
}

// values only (the sweeps read no column index): block row i holds, row by row, the rows of its nf blocks one after the other
extern "C" int tg_csr_from_blocks(int nf, const tg_csr_t *blocks, tg_csr_t *out) {
  tg_csr_s *m = new tg_csr_s;
  const int64_t n = blocks[0]->nrows;
  m->nrows = m->ncols = nf * n;
  m->rowptr = (int64_t *)malloc((nf * n + 1) * sizeof(int64_t));
  int64_t nnz = 0;
  for (int q = 0; q < nf * nf; q++) nnz += blocks[q]->nnz;
  m->nnz = nnz;
  m->val = (double *)malloc(std::max<int64_t>(nnz, 1) * sizeof(double));
  int64_t at = 0;
  for (int i = 0; i < nf; i++)
    for (int64_t r = 0; r < n; r++) {
      m->rowptr[i * n + r] = at;
      for (int j = 0; j < nf; j++) {
        const tg_csr_s *b = blocks[i * nf + j];
        for (int64_t e = b->rowptr[r]; e < b->rowptr[r + 1]; e++) m->val[at++] = b->val[e];
      }
    }
  m->rowptr[nf * n] = at;
  *out = m;
  return at == nnz ? 0 : 1;
}
