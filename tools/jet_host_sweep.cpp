// Sanitizer sweep of the second-derivative point kernels on the CPU: the kernel source of csrc/tg_jet.hip (jets of a nodal field
// and of the geometry, the transforms of point matrices and loads, the jet matrix and the jet load) and csrc/tg_shell.hip (the
// Kirchhoff-Love law), WITH their host drivers, compiled as plain C++ against tools/host_shim and run block by block with
// every array allocated at exactly its size and the LDS area poisoned beyond the size the driver asked for.  Sweeps d = 1, 2,
// every nsd >= d, p <= 4, nq = 1..10, plain and rational, nF = 1 and 3; the law with every combination of outputs, point counts
// around the workgroup size and degenerate points.  Build and run (no GPU, no Python):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -x c++ \
//           -Itools/host_shim -Iinclude tools/jet_host_sweep.cpp -o jet_host_sweep && ./jet_host_sweep
//
// Besides addresses it checks what costs nothing here (loose bounds; tests/test_gpu_jet.py and tests/test_gpu_shell.py hold
// the figures): the second derivative of a quadratic field, and the law against central differences of its own energy and
// load and for the major symmetry of its tangent.
#define TG_HOST_SWEEP_JET
#include "host_shim/tg_host_sweep.h"

static int sweep_law(long *cases) {
  const double par[3] = {1.0e3, 0.3, 0.1};
  for (int64_t npts : {1, 63, 255, 256, 257, 1000}) {
    tg_vec_s *X = vec(18 * npts, -0.3, 0.3), *U = vec(18 * npts, -0.05, 0.05);
    for (int64_t q = 0; q < npts; q++) {          // a surface close to the plane: X_,0 ~ e_0, X_,1 ~ e_1
      X->d[(6 * 0 + 1) * npts + q] += 1.0;
      X->d[(6 * 1 + 2) * npts + q] += 1.0;
    }
    for (int mask = 0; mask < 8; mask++) {
      tg_vec_s *s = (mask & 1) ? vec(18 * npts, 0.0, 0.0) : nullptr, *T = (mask & 2) ? vec(324 * npts, 0.0, 0.0) : nullptr;
      tg_vec_s *psi = (mask & 4) ? vec(npts, 0.0, 0.0) : nullptr;
      int64_t nbad = -1;
      CHECK(tg_shell_points(0, par, npts, X, U, s, T, psi, &nbad));
      if (nbad != 0) return 3;
      if ((s && !finite_all(s->d, s->n)) || (T && !finite_all(T->d, T->n)) || (psi && !finite_all(psi->d, psi->n))) return 2;
      for (tg_vec_s *v : {s, T, psi}) drop(v);
      (*cases)++;
    }
    // central differences at the first point: d psi / d jet = s, d s / d jet = T
    tg_vec_s *s = vec(18 * npts, 0.0, 0.0), *T = vec(324 * npts, 0.0, 0.0), *psi = vec(npts, 0.0, 0.0);
    int64_t nbad;
    CHECK(tg_shell_points(0, par, npts, X, U, s, T, psi, &nbad));
    const double h = 1e-5;
    for (int j = 0; j < 3; j++)
      for (int be = 0; be < 6; be++) {
        tg_vec_s *sp = vec(18 * npts, 0.0, 0.0), *sm = vec(18 * npts, 0.0, 0.0), *pp = vec(npts, 0.0, 0.0), *pm = vec(npts, 0.0, 0.0);
        double &x = U->d[(6 * j + be) * npts], x0 = x;
        x = x0 + h;
        CHECK(tg_shell_points(0, par, npts, X, U, sp, nullptr, pp, &nbad));
        x = x0 - h;
        CHECK(tg_shell_points(0, par, npts, X, U, sm, nullptr, pm, &nbad));
        x = x0;
        const double scale = 1.0 + fabs(s->d[(6 * j + be) * npts]);
        if (fabs((pp->d[0] - pm->d[0]) / (2 * h) - s->d[(6 * j + be) * npts]) > 1e-5 * scale) return 4;
        for (int i = 0; i < 3; i++)
          for (int al = 0; al < 6; al++) {
            const double t = T->d[((3 * i + j) * 36 + 6 * al + be) * npts];
            if (fabs((sp->d[(6 * i + al) * npts] - sm->d[(6 * i + al) * npts]) / (2 * h) - t) > 1e-5 * (1.0 + fabs(t)) * 10) return 5;
            if (fabs(t - T->d[((3 * j + i) * 36 + 6 * be + al) * npts]) > 1e-10 * (1.0 + fabs(t))) return 8;
          }
        for (tg_vec_s *v : {sp, sm, pp, pm}) drop(v);
      }
    for (tg_vec_s *v : {s, T, psi}) drop(v);
    // degenerate normals at known points: counted, their outputs left alone
    const int64_t bad[3] = {0, npts / 2, npts - 1};
    int64_t nb = 0;
    for (int b = 0; b < 3; b++) {
      bool seen = false;
      for (int c = 0; c < b; c++) seen = seen || bad[c] == bad[b];
      if (seen) continue;
      nb++;
      for (int c = 0; c < 3; c++) {                // x_,1 = x_,0: the current normal vanishes
        U->d[(6 * c + 2) * npts + bad[b]] = X->d[(6 * c + 1) * npts + bad[b]] + U->d[(6 * c + 1) * npts + bad[b]] - X->d[(6 * c + 2) * npts + bad[b]];
      }
    }
    s = vec(18 * npts, 0.0, 0.0), T = vec(324 * npts, 0.0, 0.0), psi = vec(npts, 0.0, 0.0);
    CHECK(tg_shell_points(0, par, npts, X, U, s, T, psi, &nbad));
    if (nbad != nb) return 6;
    if (psi->d[bad[0]] != 0.0 || s->d[npts + bad[0]] != 0.0 || T->d[7 * npts + bad[0]] != 0.0) return 7;      // (as vec() left them)
    for (tg_vec_s *v : {s, T, psi, X, U}) drop(v);
    (*cases)++;
  }
  return 0;
}

int main() {
  g_tg.ready = true;
  g_tg.host_pinned = (double *)malloc(64 * sizeof(double));
  long cases = 0;
  if (int rc = sweep_law(&cases)) {
    fprintf(stderr, "jet_host_sweep: the law failed with %d (%s)\n", rc, g_err);
    return rc;
  }
  for (int d = 1; d <= 2; d++)
    for (int nsd = d; nsd <= 3; nsd++)
      for (int p = 1; p <= 4; p++)
        for (int nq = 1; nq <= 10; nq++) {
          const int nel[2] = {d == 1 ? 3 : 2, d == 1 ? 1 : 3};
          const int nJ = d == 1 ? 3 : 6;
          std::vector<double> verts[2];
          tg_patch_t pt;
          memset(&pt, 0, sizeof(pt));
          pt.d = d, pt.p = p, pt.nsd = nsd, pt.nq = nq;
          int64_t nnodes = 1, npts = 1;
          int n[2] = {1, 1};
          for (int k = 0; k < d; k++) {
            for (int i = 0; i <= nel[k]; i++) verts[k].push_back(i * (1.0 + 0.1 * k) + 0.05 * i * i);
            pt.verts[k] = verts[k].data();
            pt.nverts[k] = nel[k] + 1;
            n[k] = nel[k] * p + 1;
            nnodes *= n[k];
            npts *= (int64_t)nel[k] * nq;
          }
          // a smooth map of the node grid with weights in [1, 1.3]; xi: the parametric coordinates of the nodes
          tg_vec_s *cp[4] = {nullptr, nullptr, nullptr, nullptr};
          for (int c = 0; c <= nsd; c++) cp[c] = vec(nnodes, 0.0, 0.0);
          tg_vec_s *uq = vec(nnodes, 0.0, 0.0);   // the quadratic field 1 + xi_0^2 (needs p >= 2 to be in the space)
          for (int64_t i = 0; i < nnodes; i++) {
            const int ik[2] = {(int)(i % n[0]), (int)(i / n[0])};
            double xi[2] = {0.0, 0.0};
            for (int k = 0; k < d; k++) {
              const int e = std::min(ik[k] / p, nel[k] - 1), a = ik[k] - e * p;
              xi[k] = verts[k][e] + (verts[k][e + 1] - verts[k][e]) * a / p;
            }
            const double w = 1.0 + 0.1 * xi[0] + 0.05 * xi[d - 1] * xi[0];
            for (int c = 0; c < nsd; c++) cp[c]->d[i] = w * (c < d ? xi[c] + 0.1 * xi[(c + 1) % d] * xi[(c + 1) % d] : 0.3 * xi[0] * xi[0] + 0.2 * xi[d - 1]);
            cp[nsd]->d[i] = w;
            uq->d[i] = 1.0 + xi[0] * xi[0];
          }
          for (int c = 0; c <= nsd; c++) pt.cp[c] = cp[c];
          for (int rat = 0; rat < 2; rat++) {
            tg_vec_s *jet = vec((int64_t)nJ * npts, 0.0, 0.0), *gj = vec((int64_t)nsd * nJ * npts, 0.0, 0.0);
            CHECK(tg_quad_jet(&pt, uq, rat, jet));
            CHECK(tg_quad_geometry_jet(&pt, gj));
            if (!finite_all(jet->d, jet->n) || !finite_all(gj->d, gj->n)) return 2;
            if (!rat && p >= 2)
              for (int64_t q = 0; q < npts; q++)
                if (fabs(jet->d[(1 + d) * npts + q] - 2.0) > 1e-9) return 9;       // d_00 (1 + xi_0^2) = 2
            drop(jet), drop(gj);
            for (int nF : {1, 3}) {
              const int64_t nb = (int64_t)nF * nF, each = (int64_t)nJ * nJ * npts;
              tg_vec_s *T = vec(nb * each, -1.0, 1.0), *coef = vec(nb * each, 0.0, 0.0);
              CHECK(tg_jet_transform(&pt, rat, (int)nb, T, coef));
              if (!finite_all(coef->d, coef->n)) return 2;
              tg_csr_t K = nullptr;
              CHECK(tg_assemble_jet_blocks(&pt, nF, coef, &K));
              if (K->nrows != nF * nnodes || !finite_all(K->val, K->nnz)) return 2;
              tg_csr_destroy(K);
              tg_vec_s *s = vec((int64_t)nF * nJ * npts, -1.0, 1.0), *st = vec((int64_t)nF * nJ * npts, 0.0, 0.0), *out = vec(nF * nnodes, 0.0, 0.0);
              CHECK(tg_jet_load_transform(&pt, rat, nF, s, st));
              CHECK(tg_quad_load_jet(&pt, nF, st, out));
              if (!finite_all(st->d, st->n) || !finite_all(out->d, out->n)) return 2;
              for (tg_vec_s *v : {T, coef, s, st, out}) drop(v);
              cases++;
            }
          }
          for (int c = 0; c <= nsd; c++) drop(cp[c]);
          drop(uq);
        }
  free(g_asm_cache.tab);
  for (int k = 0; k < 3; k++) free(g_asm_cache.verts[k]);
  free(g_tg.host_pinned);
  printf("jet_host_sweep: %ld cases (law x outputs x point counts, patches x space x fields), every entry point, largest LDS request %zu B, outputs fnv1a %016llx: clean\n",
         cases, g_host_lds_max, (unsigned long long)g_fnv);
  return 0;
}
