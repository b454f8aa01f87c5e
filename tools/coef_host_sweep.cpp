// Sanitizer sweep of the point-coefficient kernels on the CPU: the kernel source of csrc/tg_postproc.hip (coefficient
// transform, flux transform, flux load) and csrc/tg_coef.hip (plain element-matrix kernel), WITH their host drivers, compiled
// as plain C++ against tools/host_shim and run block by block with every array allocated at exactly its size and the LDS
// area poisoned beyond the size the driver asked for.  Sweeps d, nsd >= d, p <= 4, nq <= 10, plain and rational, the three
// kinds of diffusion.  Build and run (no GPU, no Python):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -x c++ \
//           -Itools/host_shim -Iinclude tools/coef_host_sweep.cpp -o coef_host_sweep && ./coef_host_sweep
//
// The sum-factorised instantiations of csrc/tg_assemble.hip use wave intrinsics and buffer instructions and are not part of
// this program (tg_asm_coef_fast is a stand-in that declines); the element-coupling pattern is rebuilt here on the host.
#include <hip/hip_runtime.h>
dim3 threadIdx, blockIdx, blockDim;
__attribute__((aligned(16))) char smem[TG_HOST_LDS_BYTES];
size_t g_host_lds_max = 0;

#include "../tigar_amd/csrc/tg_postproc.hip"
#include "../tigar_amd/csrc/tg_coef.hip"
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
  double *tab = (double *)malloc(((size_t)2 * p1 * nq + nq) * sizeof(double));      // (exactly what the kernels may read)
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

static int finite_all(const double *v, int64_t n) {
  for (int64_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return 0;
  return 1;
}

int main() {
  g_tg.ready = true;
  g_tg.host_pinned = (double *)malloc(64 * sizeof(double));
  long cases = 0;
  for (int d = 1; d <= 3; d++)
    for (int nsd = d; nsd <= 3; nsd++)
      for (int p = 1; p <= 4; p++)
        for (int nq = 1; nq <= 10; nq++) {
          if (d == 3 && (nq == 6 || nq == 8 || nq == 9)) continue;        // (3-D: 1 - 5, 7, 10)
          const int nels3[3][3] = {{3, 1, 1}, {2, 3, 1}, {2, 1, 2}};
          int nel[3] = {nels3[d - 1][0], nels3[d - 1][1], nels3[d - 1][2]};
          if (d == 3 && p >= 3 && nq >= 7) nel[0] = nel[2] = 1, nel[1] = 2;
          std::vector<double> verts[3];
          tg_patch_t pt;
          memset(&pt, 0, sizeof(pt));
          pt.d = d, pt.p = p, pt.nsd = nsd, pt.nq = nq;
          int64_t nnodes = 1, npts = 1;
          int n[3] = {1, 1, 1};
          for (int k = 0; k < d; k++) {
            for (int i = 0; i <= nel[k]; i++) verts[k].push_back(i * (1.0 + 0.1 * k) + 0.05 * i * i);
            pt.verts[k] = verts[k].data();
            pt.nverts[k] = nel[k] + 1;
            n[k] = nel[k] * p + 1;
            nnodes *= n[k];
            npts *= (int64_t)nel[k] * nq;
          }
          // a smooth map of the node grid with weights in [1, 1.3]
          tg_vec_s *cp[4] = {nullptr, nullptr, nullptr, nullptr};
          for (int c = 0; c <= nsd; c++) cp[c] = vec(nnodes, 0.0, 0.0);
          for (int64_t i = 0; i < nnodes; i++) {
            double x[3] = {(double)(i % n[0]) / p, (double)((i / n[0]) % n[1]) / p, (double)(i / ((int64_t)n[0] * n[1])) / p};
            const double w = 1.0 + 0.1 * x[0] + 0.05 * x[d - 1] * x[0];
            for (int c = 0; c < nsd; c++) cp[c]->d[i] = w * (c < d ? x[c] + 0.1 * x[(c + 1) % d] * x[(c + 1) % d] : 0.3 * x[0] * x[0] + 0.2 * x[d - 1]);
            cp[nsd]->d[i] = w;
          }
          for (int c = 0; c <= nsd; c++) pt.cp[c] = cp[c];
          const int ncomp = d * d + 2 * d + 1;
          for (int rat = 0; rat < 2; rat++)
            for (int kind = 0; kind < 3; kind++) {
              tg_vec_s *A = kind == 0 ? nullptr : vec(kind == 1 ? npts : (int64_t)nsd * nsd * npts, -1.0, 1.0);
              tg_vec_s *b = vec((int64_t)nsd * npts, -1.0, 1.0), *c = kind == 1 ? nullptr : vec((int64_t)nsd * npts, -1.0, 1.0);
              tg_vec_s *m = kind == 2 ? nullptr : vec(npts, -1.0, 1.0);
              tg_vec_s *coef = vec((int64_t)ncomp * npts, 0.0, 0.0);
              CHECK(tg_coef_transform(&pt, rat, kind, A, b, c, m, coef));
              if (!finite_all(coef->d, coef->n)) return 2;
              tg_csr_t M = nullptr;
              CHECK(tg_assemble_coef_matrix(&pt, coef, &M));
              if (!finite_all(M->val, M->nnz)) return 2;
              tg_csr_destroy(M);
              tg_vec_s *s = kind == 1 ? nullptr : vec(npts, -1.0, 1.0), *F = kind == 0 ? nullptr : vec((int64_t)nsd * npts, -1.0, 1.0);
              tg_vec_s *ft = vec((int64_t)(d + 1) * npts, 0.0, 0.0), *out = vec(nnodes, 0.0, 0.0);
              CHECK(tg_flux_transform(&pt, rat, s, F, ft));
              CHECK(rat ? tg_quad_load_flux_rational(&pt, s, F, out) : tg_quad_load_flux(&pt, s, F, out));
              if (!finite_all(ft->d, ft->n) || !finite_all(out->d, out->n)) return 2;
              for (tg_vec_s *v : {A, b, c, m, coef, s, F, ft, out}) drop(v);
              cases++;
            }
          for (int c = 0; c <= nsd; c++) drop(cp[c]);
        }
  free(g_asm_cache.tab);
  free(g_tg.host_pinned);
  printf("coef_host_sweep: %ld cases (patch x space x diffusion kind), every entry point, largest LDS request %zu B: clean\n", cases,
         g_host_lds_max);
  return 0;
}
