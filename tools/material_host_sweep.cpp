// Sanitizer sweep of the finite-strain point kernels on the CPU: the material laws of csrc/tg_material.hip, the block ending
// of k_postproc (tg_coef_transform_blocks, csrc/tg_postproc.hip) and the block driver tg_assemble_coef_blocks
// (csrc/tg_coef.hip), WITH their host drivers, compiled as plain C++ against tools/host_shim and run block by block with every
// array allocated at exactly its size and the LDS area poisoned beyond the size the driver asked for.  Sweeps d = nsd = 2, 3,
// p <= 4, nq <= 10 (as coef_host_sweep), plain and rational, with and without a reaction block, the three laws with every
// combination of outputs, point counts around the workgroup size, and states with J <= 0.  Build and run (no GPU, no Python):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -x c++ \
//           -Itools/host_shim -Iinclude tools/material_host_sweep.cpp -o material_host_sweep && ./material_host_sweep
//
// The laws are also checked here against central differences of their own energy and stress (a loose bound: this program
// checks addresses; tests/test_hyper_reference_host.py and tests/test_gpu_hyperelastic.py hold the figures).
#include "host_shim/tg_host_sweep.h"
#include "../tigar_amd/csrc/tg_material.hip"

// one law call at npts points with the outputs chosen by `mask` (1 P, 2 A, 4 psi)
static int law(int kind, int nsd, int64_t npts, tg_vec_s *H, int mask, tg_vec_s **P, tg_vec_s **A, tg_vec_s **psi, int64_t *nbad,
               double *jmin) {
  const double par[2] = {1.3, 0.7};
  const int64_t n2 = nsd * nsd;
  *P = (mask & 1) ? vec(n2 * npts, 0.0, 0.0) : nullptr;
  *A = (mask & 2) ? vec(n2 * n2 * npts, 0.0, 0.0) : nullptr;
  *psi = (mask & 4) ? vec(npts, 0.0, 0.0) : nullptr;
  CHECK(tg_material_points(kind, par, nsd, npts, H, *P, *A, *psi, nbad, jmin));
  return 0;
}

static int sweep_laws(long *cases) {
  for (int nsd = 2; nsd <= 3; nsd++)
    for (int kind = 0; kind < 3; kind++)
      for (int64_t npts : {1, 63, 255, 256, 257, 1000}) {
        const int64_t n2 = nsd * nsd;
        tg_vec_s *H = vec(n2 * npts, -0.2, 0.2);
        for (int mask = 0; mask < 8; mask++) {
          tg_vec_s *P, *A, *psi;
          int64_t nbad = -1;
          double jmin = 0.0;
          if (law(kind, nsd, npts, H, mask, &P, &A, &psi, &nbad, &jmin)) return 1;
          if (nbad != 0 || !(jmin > 0.0 && jmin < 3.0)) return 3;
          if ((P && !finite_all(P->d, P->n)) || (A && !finite_all(A->d, A->n)) || (psi && !finite_all(psi->d, psi->n))) return 2;
          for (tg_vec_s *v : {P, A, psi}) drop(v);
          (*cases)++;
        }
        // central differences at the first point: dpsi / dF = P, dP / dF = A
        tg_vec_s *P, *A, *psi;
        int64_t nbad;
        double jmin;
        if (law(kind, nsd, npts, H, 7, &P, &A, &psi, &nbad, &jmin)) return 1;
        const double h = 1e-5;
        for (int j = 0; j < nsd; j++)
          for (int L = 0; L < nsd; L++) {
            tg_vec_s *Pp, *Ap, *sp, *Pm, *Am, *sm;
            double &x = H->d[(j * nsd + L) * npts], x0 = x;
            x = x0 + h;
            if (law(kind, nsd, npts, H, 5, &Pp, &Ap, &sp, &nbad, &jmin)) return 1;
            x = x0 - h;
            if (law(kind, nsd, npts, H, 5, &Pm, &Am, &sm, &nbad, &jmin)) return 1;
            x = x0;
            if (fabs((sp->d[0] - sm->d[0]) / (2 * h) - P->d[(j * nsd + L) * npts]) > 1e-6) return 4;
            for (int i = 0; i < nsd; i++)
              for (int K = 0; K < nsd; K++)
                if (fabs((Pp->d[(i * nsd + K) * npts] - Pm->d[(i * nsd + K) * npts]) / (2 * h) -
                         A->d[(((i * nsd + j) * nsd + K) * nsd + L) * npts]) > 1e-6)
                  return 5;
            for (tg_vec_s *v : {Pp, sp, Pm, sm}) drop(v);
          }
        for (tg_vec_s *v : {P, A, psi}) drop(v);
        // J <= 0 at known points: kind 2 counts them and leaves their outputs alone, the others compute
        const int64_t bad[3] = {0, npts / 2, npts - 1};
        int64_t nb = 0;
        for (int b = 0; b < 3; b++) {
          bool seen = false;
          for (int c = 0; c < b; c++) seen = seen || bad[c] == bad[b];
          if (seen) continue;
          nb++;
          for (int i = 0; i < nsd; i++)
            for (int K = 0; K < nsd; K++) H->d[(i * nsd + K) * npts + bad[b]] = i == K ? (i == 0 ? -2.5 : 0.0) : 0.0;      // F = diag(-1.5, 1, ..)
        }
        if (law(kind, nsd, npts, H, 7, &P, &A, &psi, &nbad, &jmin)) return 1;
        if (nbad != (kind == 2 ? nb : 0) || jmin != -1.5) return 6;
        if (kind == 2 && (psi->d[bad[0]] != 0.0 || P->d[bad[0]] != 0.0 || A->d[bad[0]] != 0.0)) return 7;   // (as vec() left them)
        for (tg_vec_s *v : {P, A, psi, H}) drop(v);
        (*cases)++;
      }
  return 0;
}

int main() {
  g_tg.ready = true;
  g_tg.host_pinned = (double *)malloc(64 * sizeof(double));
  long cases = 0;
  if (int rc = sweep_laws(&cases)) {
    fprintf(stderr, "material_host_sweep: the laws failed with %d (%s)\n", rc, g_err);
    return rc;
  }
  for (int d = 2; d <= 3; d++)
    for (int p = 1; p <= 4; p++)
      for (int nq = 1; nq <= 10; nq++) {
        if (d == 3 && (nq == 6 || nq == 8 || nq == 9)) continue;        // (3-D: 1 - 5, 7, 10)
        int nel[3] = {d == 2 ? 2 : 2, d == 2 ? 3 : 1, d == 2 ? 1 : 2};
        if (d == 3 && p >= 3 && nq >= 7) nel[0] = nel[2] = 1, nel[1] = 2;
        std::vector<double> verts[3];
        tg_patch_t pt;
        memset(&pt, 0, sizeof(pt));
        pt.d = d, pt.p = p, pt.nsd = d, pt.nq = nq;
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
        for (int c = 0; c <= d; c++) cp[c] = vec(nnodes, 0.0, 0.0);
        for (int64_t i = 0; i < nnodes; i++) {
          double x[3] = {(double)(i % n[0]) / p, (double)((i / n[0]) % n[1]) / p, (double)(i / ((int64_t)n[0] * n[1])) / p};
          const double w = 1.0 + 0.1 * x[0] + 0.05 * x[d - 1] * x[0];
          for (int c = 0; c < d; c++) cp[c]->d[i] = w * (x[c] + 0.1 * x[(c + 1) % d] * x[(c + 1) % d]);
          cp[d]->d[i] = w;
        }
        for (int c = 0; c <= d; c++) pt.cp[c] = cp[c];
        const int64_t ncomp = d * d + 2 * d + 1, nb = d * d;
        for (int rat = 0; rat < 2; rat++)
          for (int react = 0; react < 2; react++) {
            // the tangent of the neo-Hookean law at a random state, as a Newton step produces it
            tg_vec_s *H = vec(nb * npts, -0.2, 0.2), *P, *A, *psi;
            int64_t nbad;
            double jmin;
            if (law(2, d, npts, H, 2, &P, &A, &psi, &nbad, &jmin)) return 1;
            tg_vec_s *M = react ? vec(nb * npts, -1.0, 1.0) : nullptr;
            tg_vec_s *coef = vec(nb * ncomp * npts, 0.0, 0.0);
            CHECK(tg_coef_transform_blocks(&pt, rat, d, A, M, coef));
            if (!finite_all(coef->d, coef->n)) return 2;
            tg_csr_t K = nullptr;
            CHECK(tg_assemble_coef_blocks(&pt, d, coef, &K));
            if (K->nrows != d * nnodes || !finite_all(K->val, K->nnz)) return 2;
            tg_csr_destroy(K);
            for (tg_vec_s *v : {H, A, M, coef}) drop(v);
            cases++;
          }
        for (int c = 0; c <= d; c++) drop(cp[c]);
      }
  free(g_asm_cache.tab);
  free(g_tg.host_pinned);
  printf("material_host_sweep: %ld cases (laws x outputs x point counts, patches x space x reaction), largest LDS request %zu B, outputs fnv1a %016llx: clean\n",
         cases, g_host_lds_max, (unsigned long long)g_fnv);
  return 0;
}
