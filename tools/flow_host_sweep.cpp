// Sanitizer sweep of the flow point kernels on the CPU: the law of csrc/tg_flow.hip, the block ending of k_postproc with b and c
// per block (tg_coef_transform_system), the metric ending (tg_quad_metric, csrc/tg_postproc.hip) and the block driver
// tg_assemble_coef_system (csrc/tg_coef.hip), WITH their host drivers, compiled as plain C++ against tools/host_shim and run
// block by block with every array allocated at exactly its size and the LDS area poisoned beyond the size the driver asked
// for.  Sweeps the law at nsd = 2, 3 with 1, 63, 255, 256, 257 and 1000 points and every subset of its seven outputs, with and
// without a0 and f; the system transform at d = 1, 2, 3 (nsd = d, and a surface in space), p <= 4, nF = 1, 2, 4, plain and
// rational, every subset of the four terms.  Build and run (no GPU, no Python):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -x c++ \
//           -Itools/host_shim -Iinclude tools/flow_host_sweep.cpp -o flow_host_sweep && ./flow_host_sweep
//
// The tangent is also checked here against central differences of the law's own source and flux (a loose bound: this program
// checks addresses; tests/test_flow_reference_host.py and tests/test_gpu_flow.py hold the figures).
#include "host_shim/tg_host_sweep.h"
#include "../tigar_amd/csrc/tg_flow.hip"

static const double PAR[5] = {1.3, 0.2, 1.7, 64.0, 36.0};

struct flow_out {
  tg_vec_s *v[7];        // s, F, A, b, c, M, tau
};

static int law(int nsd, int64_t npts, tg_vec_s *U, tg_vec_s *gU, tg_vec_s *a0, tg_vec_s *f, tg_vec_s *G, int mask, flow_out *o) {
  const int64_t nF = nsd + 1, each[7] = {nF, nF * nsd, nF * nF * nsd * nsd, nF * nF * nsd, nF * nF * nsd, nF * nF, 2};
  for (int k = 0; k < 7; k++) o->v[k] = (mask >> k & 1) ? vec(each[k] * npts, 0.0, 0.0) : nullptr;
  CHECK(tg_flow_points(PAR, nsd, npts, U, gU, a0, f, G, o->v[0], o->v[1], o->v[2], o->v[3], o->v[4], o->v[5], o->v[6]));
  return 0;
}

static void drop(flow_out *o) {
  for (int k = 0; k < 7; k++) drop(o->v[k]);
}

static int sweep_law(long *cases) {
  for (int nsd = 2; nsd <= 3; nsd++)
    for (int64_t npts : {1, 63, 255, 256, 257, 1000}) {
      const int64_t nF = nsd + 1;
      tg_vec_s *U = vec(nF * npts, -1.0, 1.0), *gU = vec(nF * nsd * npts, -1.0, 1.0), *a0 = vec(nsd * npts, -1.0, 1.0),
               *f = vec(nsd * npts, -1.0, 1.0), *G = vec((int64_t)nsd * nsd * npts, -0.5, 0.5);
      for (int64_t q = 0; q < npts; q++)                                 // a symmetric, diagonally dominant metric
        for (int K = 0; K < nsd; K++) {
          G->d[(K * nsd + K) * npts + q] = 4.0 + fabs(G->d[(K * nsd + K) * npts + q]);
          for (int L = 0; L < K; L++) G->d[(K * nsd + L) * npts + q] = G->d[(L * nsd + K) * npts + q];
        }
      for (int with = 0; with < 2; with++)
        for (int mask = 0; mask < 128; mask++) {
          flow_out o;
          if (law(nsd, npts, U, gU, with ? a0 : nullptr, with ? f : nullptr, G, mask, &o)) return 1;
          for (int k = 0; k < 7; k++)
            if (o.v[k] && !finite_all(o.v[k]->d, o.v[k]->n)) return 2;
          drop(&o);
          (*cases)++;
        }
      // central differences at the last point: d (s, F) / d U_j = (m, b), d (s, F) / d (d_L U_j) = (c, A)
      flow_out o;
      if (law(nsd, npts, U, gU, a0, f, G, 127, &o)) return 1;
      const double h = 1e-5;
      const int64_t q = npts - 1;
      for (int64_t i = 0; i < npts; i++)                                 // every point was written (vec() left zeros)
        if (!(o.v[6]->d[i] > 0.0 && o.v[6]->d[npts + i] > 0.0)) return 7;
      for (int j = 0; j < nF; j++)
        for (int L = -1; L < nsd; L++) {
          double &x = L < 0 ? U->d[j * npts + q] : gU->d[(j * nsd + L) * npts + q], x0 = x;
          flow_out op, om;
          x = x0 + h;
          if (law(nsd, npts, U, gU, a0, f, G, 3, &op)) return 1;
          x = x0 - h;
          if (law(nsd, npts, U, gU, a0, f, G, 3, &om)) return 1;
          x = x0;
          for (int i = 0; i < nF; i++) {
            const double ds = (op.v[0]->d[i * npts + q] - om.v[0]->d[i * npts + q]) / (2 * h);
            const double ws = L < 0 ? o.v[5]->d[(i * nF + j) * npts + q] : o.v[4]->d[((i * nF + j) * nsd + L) * npts + q];
            if (fabs(ds - ws) > 1e-6) return 4;
            for (int K = 0; K < nsd; K++) {
              const double dF = (op.v[1]->d[(i * nsd + K) * npts + q] - om.v[1]->d[(i * nsd + K) * npts + q]) / (2 * h);
              const double wF = L < 0 ? o.v[3]->d[((i * nF + j) * nsd + K) * npts + q]
                                      : o.v[2]->d[(((i * nF + j) * nsd + K) * nsd + L) * npts + q];
              if (fabs(dF - wF) > 1e-6) return 5;
            }
          }
          drop(&op);
          drop(&om);
        }
      drop(&o);
      // wrong sizes and parameters are refused before a launch
      tg_vec_s *shortU = vec(nF * npts - 1, 0.0, 0.0);
      const double bad[5] = {0.0, 0.2, 0.0, 0.0, 36.0};
      if (tg_flow_points(PAR, nsd, npts, shortU, gU, nullptr, nullptr, G, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 ||
          tg_flow_points(bad, nsd, npts, U, gU, nullptr, nullptr, G, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 ||
          tg_flow_points(PAR, 4, npts, U, gU, nullptr, nullptr, G, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0)
        return 6;
      for (tg_vec_s *v : {U, gU, a0, f, G, shortU}) drop(v);
    }
  return 0;
}

// one patch: d parametric directions in nsd physical ones, nel elements per direction
static int sweep_patch(int d, int nsd, int p, int nq, const int *nel, long *cases) {
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
  tg_vec_s *cp[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int c = 0; c <= nsd; c++) cp[c] = vec(nnodes, 0.0, 0.0);
  for (int64_t i = 0; i < nnodes; i++) {
    double x[3] = {(double)(i % n[0]) / p, (double)((i / n[0]) % n[1]) / p, (double)(i / ((int64_t)n[0] * n[1])) / p};
    const double w = 1.0 + 0.1 * x[0] + 0.05 * x[d - 1] * x[0];
    for (int c = 0; c < d; c++) cp[c]->d[i] = w * (x[c] + 0.1 * x[(c + 1) % d] * x[(c + 1) % d]);
    for (int c = d; c < nsd; c++) cp[c]->d[i] = w * (0.3 * x[0] * x[0] - 0.2 * x[d - 1]);      // out of the parameter space
    cp[nsd]->d[i] = w;
  }
  for (int c = 0; c <= nsd; c++) pt.cp[c] = cp[c];
  const int64_t ncomp = d * d + 2 * d + 1;
  tg_vec_s *G = vec((int64_t)nsd * nsd * npts, 0.0, 0.0);
  CHECK(tg_quad_metric(&pt, G));
  if (!finite_all(G->d, G->n)) return 2;
  drop(G);
  (*cases)++;
  for (int nF : {1, 2, 4}) {
    const int64_t nb = (int64_t)nF * nF;
    tg_vec_s *A = vec(nb * nsd * nsd * npts, -1.0, 1.0), *b = vec(nb * nsd * npts, -1.0, 1.0), *c = vec(nb * nsd * npts, -1.0, 1.0),
             *M = vec(nb * npts, -1.0, 1.0);
    for (int rat = 0; rat < 2; rat++)
      for (int mask = 0; mask < 16; mask++) {
        tg_vec_s *coef = vec(nb * ncomp * npts, 0.0, 0.0);
        CHECK(tg_coef_transform_system(&pt, rat, nF, mask & 1 ? A : nullptr, mask & 2 ? b : nullptr, mask & 4 ? c : nullptr,
                                       mask & 8 ? M : nullptr, coef));
        if (!finite_all(coef->d, coef->n)) return 2;
        if (mask == 15 || mask == 6) {
          tg_csr_t K = nullptr;
          CHECK(tg_assemble_coef_system(&pt, nF, coef, &K));
          if (K->nrows != nF * nnodes || !finite_all(K->val, K->nnz)) return 2;
          tg_csr_destroy(K);
        }
        drop(coef);
        (*cases)++;
      }
    // a term of the wrong size, too many fields
    tg_vec_s *coef = vec(nb * ncomp * npts, 0.0, 0.0), *shortb = vec(nb * nsd * npts - 1, 0.0, 0.0);
    if (tg_coef_transform_system(&pt, 0, nF, A, shortb, c, M, coef) == 0 || tg_coef_transform_system(&pt, 0, 17, A, b, c, M, coef) == 0) return 6;
    for (tg_vec_s *v : {A, b, c, M, coef, shortb}) drop(v);
  }
  for (int c = 0; c <= nsd; c++) drop(cp[c]);
  return 0;
}

int main() {
  g_tg.ready = true;
  g_tg.host_pinned = (double *)malloc(64 * sizeof(double));
  long cases = 0;
  if (int rc = sweep_law(&cases)) {
    fprintf(stderr, "flow_host_sweep: the law failed with %d (%s)\n", rc, g_err);
    return rc;
  }
  for (int d = 1; d <= 3; d++)
    for (int p = 1; p <= 4; p++)
      for (int nq : {1, p + 1, p + 2, 10}) {
        if (d == 3 && nq == 10 && p >= 3) continue;                    // (one element of these is what material_host_sweep runs)
        const int nel2[3] = {2, 3, 1}, nel3[3] = {2, 1, 2}, nel1[3] = {5, 1, 1};
        const int *nel = d == 1 ? nel1 : (d == 2 ? nel2 : nel3);
        if (int rc = sweep_patch(d, d, p, nq, nel, &cases)) {
          fprintf(stderr, "flow_host_sweep: d = %d, p = %d, nq = %d failed with %d (%s)\n", d, p, nq, rc, g_err);
          return rc;
        }
        if (d < 3)                                                       // a curve in the plane, a surface in space
          if (int rc = sweep_patch(d, d + 1, p, nq, nel, &cases)) {
            fprintf(stderr, "flow_host_sweep: d = %d, nsd = %d, p = %d, nq = %d failed with %d (%s)\n", d, d + 1, p, nq, rc, g_err);
            return rc;
          }
      }
  free(g_asm_cache.tab);
  free(g_tg.host_pinned);
  printf("flow_host_sweep: %ld cases (law x outputs x point counts, patches x fields x space x terms), largest LDS request %zu B, "
         "outputs fnv1a %016llx: clean\n", cases, g_host_lds_max, (unsigned long long)g_fnv);
  return 0;
}
