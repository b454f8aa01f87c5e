// Sanitizer sweep of the point kernels of csrc/tg_sample.hip and of the lattice entry points of csrc/tg_postproc.hip on the CPU:
// the kernel source WITH its host drivers, compiled as plain C++ against tools/host_shim and run block by block with every
// array allocated at exactly its size and the LDS area (the seed tiles, the per-lane tables of the generic route) poisoned
// beyond the size the driver asked for.  Sweeps tg_point_eval over d = 1, 2, 3, p = 1..4 (and 5, 8 where (p+1)^d fits: the
// generic route), nsd = d and d + 1, nF = 1 and 3, plain and rational, every subset of the three outputs, with and without
// the nodal vector, 0, 1, 63, 64, 65, 257 and 1500 points (more than the capped grid has workgroups: the stride loop) that lie
// inside, on element vertices, on the ends, outside, and are not finite; tg_point_locate with and without a guess, with 1, 7 and
// all seeds (more than one tile of them), 0, 1, 65 and 257 points, a NaN point and the iteration limit; the lattice entries
// at m = 1, 2, p + 1, 10 with and without the ends.  Build and run (no GPU, no Python):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -x c++ \
//           -Itools/host_shim -Iinclude tools/sample_host_sweep.cpp -o sample_host_sweep && ./sample_host_sweep
//
// The shim runs ONE thread per workgroup: the lane-strided tables of the generic route are then addressed at lane 0 only, so
// "exactly their size" holds for the global arrays and the seed tiles, not for the 2 d (p + 1) 64 doubles of that table area
// (its indexing (2 k (p + 1) + a) nt + lane < 2 d (p + 1) nt is read off the source).
// Figures are checked loosely (this program checks addresses; tests/test_gpu_sample.py holds the bounds): a polynomial of
// degree p in the knot coordinates comes back at the points, outside points give NaN and nothing else does, x = F(xi) is
// found again by the projection.
#define TG_HOST_SWEEP_SAMPLE
#include "host_shim/tg_host_sweep.h"

struct patch_t {
  tg_patch_t pt;
  std::vector<double> verts[3];
  tg_vec_s *cp[4] = {nullptr, nullptr, nullptr, nullptr};
  int n[3] = {1, 1, 1};
  int64_t nnodes = 1;
  std::vector<double> node_xi[3];      // knot coordinates of the nodes per direction
};

static void make_patch(patch_t *P, int d, int nsd, int p, const int *nel) {
  memset(&P->pt, 0, sizeof(P->pt));
  P->pt.d = d, P->pt.p = p, P->pt.nsd = nsd, P->pt.nq = 0;        // (nq is not read by the sampling entries)
  P->nnodes = 1;
  for (int k = 0; k < 3; k++) P->n[k] = 1;
  for (int k = 0; k < d; k++) {
    P->verts[k].clear();
    P->node_xi[k].clear();
    for (int i = 0; i <= nel[k]; i++) P->verts[k].push_back(0.25 + i * (1.0 + 0.1 * k) + 0.05 * i * i);
    for (int e = 0; e < nel[k]; e++)
      for (int a = (e ? 1 : 0); a <= p; a++) P->node_xi[k].push_back(P->verts[k][e] + (P->verts[k][e + 1] - P->verts[k][e]) * a / p);
    P->pt.verts[k] = P->verts[k].data();
    P->pt.nverts[k] = nel[k] + 1;
    P->n[k] = nel[k] * p + 1;
    P->nnodes *= P->n[k];
  }
  for (int c = 0; c <= nsd; c++) P->cp[c] = vec(P->nnodes, 0.0, 0.0);
  for (int64_t i = 0; i < P->nnodes; i++) {
    const int id[3] = {(int)(i % P->n[0]), (int)((i / P->n[0]) % P->n[1]), (int)(i / ((int64_t)P->n[0] * P->n[1]))};
    double x[3] = {0, 0, 0};
    for (int k = 0; k < d; k++) x[k] = P->node_xi[k][id[k]];
    const double w = 1.0 + 0.05 * x[0] + 0.02 * x[d - 1] * x[0];
    for (int c = 0; c < d; c++) P->cp[c]->d[i] = w * (x[c] + 0.02 * x[(c + 1) % d] * x[(c + 1) % d]);
    for (int c = d; c < nsd; c++) P->cp[c]->d[i] = w * (0.05 * x[0] * x[0] - 0.2 * x[d - 1]);
    P->cp[nsd]->d[i] = w;
  }
  for (int c = 0; c <= nsd; c++) P->pt.cp[c] = P->cp[c];
}

static void drop_patch(patch_t *P) {
  for (int c = 0; c < 4; c++) {
    drop(P->cp[c]);
    P->cp[c] = nullptr;
  }
}

// a polynomial of degree p per direction in the knot coordinates
static double poly(int d, int p, int field, const double *xi) {
  double v = 1.0 + field;
  for (int k = 0; k < d; k++) v *= 0.5 + pow(0.3 * xi[k], p) - 0.1 * (k + field) * xi[k];
  return v;
}

// the points of a sweep: inside, on vertices, on the ends, outside, not finite -- by the index of the point
static void make_points(const patch_t &P, int64_t npts, tg_vec_s *xi, std::vector<char> *inside) {
  const int d = P.pt.d;
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  inside->assign(npts, 1);
  for (int64_t q = 0; q < npts; q++) {
    for (int k = 0; k < d; k++) {
      const std::vector<double> &v = P.verts[k];
      const double lo = v.front(), hi = v.back();
      double x = lo + (hi - lo) * u01(g_rng);
      switch ((q + 3 * k) % 11) {
        case 1: x = v[(size_t)(u01(g_rng) * v.size()) % v.size()]; break;      // on a vertex
        case 2: x = lo; break;
        case 3: x = hi; break;
        case 4: x = std::nextafter(hi, 2.0 * hi); break;                        // one ulp outside
        case 5: x = std::nextafter(lo, -1.0); break;
        case 6: x = std::nextafter(hi, lo); break;                              // one ulp inside
        case 7: x = (q % 3 == 0) ? NAN : (q % 3 == 1 ? INFINITY : -INFINITY); break;
        case 8: x = hi + 1.0; break;
        default: break;
      }
      xi->d[k * npts + q] = x;
      if (!(x >= lo && x <= hi)) (*inside)[q] = 0;
    }
  }
}

static int sweep_eval(int d, int nsd, int p, const int *nel, long *cases) {
  patch_t P;
  make_patch(&P, d, nsd, p, nel);
  for (int nF : {1, 3}) {
    tg_vec_s *u = vec(nF * P.nnodes, 0.0, 0.0);
    for (int f = 0; f < nF; f++)
      for (int64_t i = 0; i < P.nnodes; i++) {
        const int id[3] = {(int)(i % P.n[0]), (int)((i / P.n[0]) % P.n[1]), (int)(i / ((int64_t)P.n[0] * P.n[1]))};
        double x[3] = {0, 0, 0};
        for (int k = 0; k < d; k++) x[k] = P.node_xi[k][id[k]];
        u->d[f * P.nnodes + i] = poly(d, p, f, x);
      }
    for (int64_t npts : {0, 1, 63, 64, 65, 257, 1500}) {
      if (npts == 1500 && nF == 3) continue;
      tg_vec_s *xi = vec(d * npts, 0.0, 0.0);
      std::vector<char> inside;
      make_points(P, npts, xi, &inside);
      for (int rat = 0; rat < 2; rat++)
        for (int mask = 0; mask < 8; mask++)
          for (int with_u = 0; with_u < 2; with_u++) {
            if (!with_u && (mask & 6)) continue;                                // (values need a nodal vector: refused, below)
            tg_vec_s *x = (mask & 1) ? vec(nsd * npts, 7.0, 7.0) : nullptr, *val = (mask & 2) ? vec(nF * npts, 7.0, 7.0) : nullptr,
                     *grad = (mask & 4) ? vec((int64_t)nF * nsd * npts, 7.0, 7.0) : nullptr;
            CHECK(tg_point_eval(&P.pt, nF, with_u ? u : nullptr, xi, rat, x, val, grad));
            for (int64_t q = 0; q < npts; q++) {
              for (int c = 0; x && c < nsd; c++)
                if ((bool)std::isfinite(x->d[c * npts + q]) != (bool)inside[q]) return 2;
              for (int f = 0; val && f < nF; f++) {
                const double v = val->d[f * npts + q];
                if ((bool)std::isfinite(v) != (bool)inside[q]) return 2;
                if (inside[q] && !rat) {
                  double xq[3] = {0, 0, 0};
                  for (int k = 0; k < d; k++) xq[k] = xi->d[k * npts + q];
                  if (fabs(v - poly(d, p, f, xq)) > 1e-9 * (1.0 + fabs(v))) return 3;
                }
              }
              for (int64_t j = 0; grad && j < (int64_t)nF * nsd; j++)
                if ((bool)std::isfinite(grad->d[j * npts + q]) != (bool)inside[q]) return 2;
            }
            for (tg_vec_s *v : {x, val, grad})
              if (v) (void)finite_all(v->d, v->n);
            for (tg_vec_s *v : {x, val, grad}) drop(v);
            (*cases)++;
          }
      // refusals: values without a nodal vector, outputs of the wrong size, a nodal vector of the wrong size
      tg_vec_s *val = vec(nF * npts, 0.0, 0.0), *shortx = vec(nsd * npts + 1, 0.0, 0.0), *shortu = vec(nF * P.nnodes - 1, 0.0, 0.0);
      if (tg_point_eval(&P.pt, nF, nullptr, xi, 0, nullptr, val, nullptr) == 0 || tg_point_eval(&P.pt, nF, u, xi, 0, shortx, nullptr, nullptr) == 0 ||
          tg_point_eval(&P.pt, nF, shortu, xi, 0, nullptr, val, nullptr) == 0 || tg_point_eval(&P.pt, 0, u, xi, 0, nullptr, nullptr, nullptr) == 0)
        return 6;
      for (tg_vec_s *v : {val, shortx, shortu, xi}) drop(v);
    }
    drop(u);
  }
  drop_patch(&P);
  return 0;
}

static int sweep_locate(int d, int nsd, int p, const int *nel, long *cases) {
  patch_t P;
  make_patch(&P, d, nsd, p, nel);
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  for (int64_t npts : {0, 1, 65, 257}) {
    tg_vec_s *xi = vec(d * npts, 0.0, 0.0), *x = vec(nsd * npts, 0.0, 0.0);
    for (int64_t q = 0; q < npts; q++)
      for (int k = 0; k < d; k++) {
        const double lo = P.verts[k].front(), hi = P.verts[k].back();
        xi->d[k * npts + q] = q % 5 == 0 ? (q % 2 ? lo : hi) : lo + (hi - lo) * u01(g_rng);     // a fifth of them on faces
      }
    CHECK(tg_point_eval(&P.pt, 1, nullptr, xi, 0, x, nullptr, nullptr));
    if (npts > 2) x->d[2] = NAN;                                                                // one point is not finite
    for (int with_guess = 0; with_guess < 2; with_guess++)
      for (int64_t max_seeds : {(int64_t)1, (int64_t)7, (int64_t)32768})
        for (int max_iter : {1, 50}) {
          if (with_guess && max_seeds != 1) continue;
          tg_vec_s *guess = nullptr;
          if (with_guess) {
            guess = vec(d * npts, 0.0, 0.0);
            for (int64_t q = 0; q < npts; q++)
              for (int k = 0; k < d; k++)                                                       // near the answer, some outside the box
                guess->d[k * npts + q] = xi->d[k * npts + q] + 0.3 * (u01(g_rng) - 0.5);
          }
          tg_vec_s *out = vec(d * npts, 7.0, 7.0), *info = vec(3 * npts, 7.0, 7.0);
          CHECK(tg_point_locate(&P.pt, x, guess, 1e-12, max_iter, max_seeds, out, info));
          for (int64_t q = 0; q < npts; q++) {
            const int status = (int)info->d[2 * npts + q];
            if (q == 2) {
              if (status != 2 || !std::isnan(out->d[q])) return 4;
              continue;
            }
            if (status != 0 && status != 1) return 4;
            if (max_iter == 1 && info->d[npts + q] != 1.0) return 4;
            for (int k = 0; k < d; k++) {
              const double v = out->d[k * npts + q];
              if (!(v >= P.verts[k].front() && v <= P.verts[k].back())) return 5;               // always inside the box
              if (max_iter == 50 && nsd == d && max_seeds > 7 && status == 0 && nel[0] < 20 && fabs(v - xi->d[k * npts + q]) > 1e-9) return 3;
            }
          }
          (void)finite_all(info->d, info->n);
          for (tg_vec_s *v : {guess, out, info}) drop(v);
          (*cases)++;
        }
    // refusals
    tg_vec_s *out = vec(d * npts, 0.0, 0.0), *info = vec(3 * npts, 0.0, 0.0), *shortinfo = vec(3 * npts + 1, 0.0, 0.0);
    if (tg_point_locate(&P.pt, x, nullptr, 0.0, 50, 1, out, info) == 0 || tg_point_locate(&P.pt, x, nullptr, 1e-12, 101, 1, out, info) == 0 ||
        tg_point_locate(&P.pt, x, nullptr, 1e-12, 0, 1, out, info) == 0 || tg_point_locate(&P.pt, x, nullptr, 1e-12, 50, 0, out, info) == 0 ||
        tg_point_locate(&P.pt, x, nullptr, 1e-12, 50, 1, out, shortinfo) == 0)
      return 6;
    for (tg_vec_s *v : {xi, x, out, info, shortinfo}) drop(v);
  }
  drop_patch(&P);
  return 0;
}

static int sweep_lattice(int d, int nsd, int p, const int *nel, long *cases) {
  patch_t P;
  make_patch(&P, d, nsd, p, nel);
  tg_vec_s *u = vec(P.nnodes, -1.0, 1.0);
  for (int m : {1, 2, p + 1, 10})
    for (int ends = 0; ends < 2; ends++) {
      if (d == 3 && m == 10 && p >= 3) continue;                          // (one element of these: material_host_sweep's shapes)
      std::vector<double> t(m);                                            // exactly m abscissae
      for (int q = 0; q < m; q++) t[q] = ends ? (m == 1 ? 1.0 : (double)q / (m - 1)) : (q + 0.5) / m;
      int64_t npts = 1;
      for (int k = 0; k < d; k++) npts *= (int64_t)nel[k] * m;
      tg_vec_s *x = vec(nsd * npts, 0.0, 0.0);
      CHECK(tg_lattice_points(&P.pt, m, t.data(), x));
      if (!finite_all(x->d, x->n)) return 2;
      for (int rat = 0; rat < 2; rat++)
        for (int with_grad = 0; with_grad < 2; with_grad++) {
          tg_vec_s *val = vec(npts, 0.0, 0.0), *grad = with_grad ? vec(nsd * npts, 0.0, 0.0) : nullptr;
          CHECK((rat ? tg_lattice_eval_rational : tg_lattice_eval)(&P.pt, m, t.data(), u, with_grad, val, grad));
          if (!finite_all(val->d, val->n) || (grad && !finite_all(grad->d, grad->n))) return 2;
          drop(val);
          drop(grad);
          (*cases)++;
        }
      const double bad[2] = {0.5, 0.5}, out_of_range[1] = {1.5};
      if (tg_lattice_points(&P.pt, 2, bad, x) == 0 || tg_lattice_points(&P.pt, 1, out_of_range, x) == 0 ||
          tg_lattice_points(&P.pt, 11, t.data(), x) == 0 || tg_lattice_points(&P.pt, 0, t.data(), x) == 0)
        return 6;
      drop(x);
      (*cases)++;
    }
  drop(u);
  drop_patch(&P);
  return 0;
}

int main() {
  g_tg.ready = true;
  g_tg.host_pinned = (double *)malloc(64 * sizeof(double));
  long cases = 0;
  const int nel1[3] = {7, 1, 1}, nel2[3] = {3, 2, 1}, nel2b[3] = {1, 7, 1}, nel3[3] = {2, 1, 3}, one[3] = {1, 1, 1}, many[3] = {20, 15, 1};
  for (int d = 1; d <= 3; d++)
    for (int p : {1, 2, 3, 4, 5, 8}) {
      int nloc = 1;
      for (int k = 0; k < d; k++) nloc *= p + 1;
      if (nloc > TG_ASM_MAXLOC) continue;
      for (int nsd = d; nsd <= std::min(3, d + 1); nsd++)
        for (const int *nel : {d == 1 ? nel1 : (d == 2 ? nel2 : nel3), one, nel2b}) {
          if (nel == nel2b && d != 2) continue;
          int rc = sweep_eval(d, nsd, p, nel, &cases);
          if (!rc && nel != one) rc = sweep_locate(d, nsd, p, nel, &cases);
          if (!rc && nel != nel2b && p <= 4) rc = sweep_lattice(d, nsd, p, nel, &cases);
          if (rc) {
            fprintf(stderr, "sample_host_sweep: d = %d, nsd = %d, p = %d, %d x %d x %d elements failed with %d (%s)\n", d, nsd, p, nel[0],
                    nel[1], nel[2], rc, g_err);
            return rc;
          }
        }
    }
  // more seeds than one tile holds (300 elements), and a stride that leaves a partial tile
  if (int rc = sweep_locate(2, 2, 2, many, &cases)) {
    fprintf(stderr, "sample_host_sweep: the seed tiles failed with %d (%s)\n", rc, g_err);
    return rc;
  }
  free(g_asm_cache.tab);
  free(g_tg.host_pinned);
  printf("sample_host_sweep: %ld cases (patches x fields x space x outputs x point counts; projections; lattices), largest LDS "
         "request %zu B, outputs fnv1a %016llx: clean\n", cases, g_host_lds_max, (unsigned long long)g_fnv);
  return 0;
}
