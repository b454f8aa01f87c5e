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
#include "host_shim/tg_host_sweep.h"

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
  printf("coef_host_sweep: %ld cases (patch x space x diffusion kind), every entry point, largest LDS request %zu B, outputs fnv1a %016llx: clean\n",
         cases, g_host_lds_max, (unsigned long long)g_fnv);
  return 0;
}
