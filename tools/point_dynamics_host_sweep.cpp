// Sanitizer sweep of the point kernel of structural dynamics (tg_point_dynamics, csrc/tg_dynamics.hip) on the CPU: the kernel
// source WITH its host driver, compiled as plain C++ against tools/host_shim and run block by block with every array
// allocated at exactly its size.  Sweeps every (nF, nJ), point counts around the workgroup size, every subset of the optional
// arguments {u, w, plane, s, T, e_out, nactive}, sigma = 1 and sigma != 1, and planes with all, no and some points active.
// Build and run (no GPU, no Python):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -x c++ \
//           -Itools/host_shim -Iinclude tools/point_dynamics_host_sweep.cpp -o point_dynamics_host_sweep && ./point_dynamics_host_sweep
//
// Besides addresses it checks what costs nothing here: every output against the formulas written out in long double (loose
// bound; tests/test_gpu_dynamics.py holds the figures), the count of active points, that points with g = 0 exactly are
// inactive, that every entry of s and T the kernel has no business with keeps its bits, and what the driver refuses.
#include "host_shim/tg_host_sweep.h"
#include "../tigar_amd/csrc/tg_dynamics.hip"
#include <vector>

static const int64_t kCounts[] = {1, 63, 255, 256, 257, 1000};
static const int kShapes[][2] = {{2, 1}, {2, 3}, {2, 6}, {3, 1}, {3, 3}, {3, 6}};

static bool near(double got, long double want, long double mag) { return fabsl((long double)got - want) <= 1e-13L * (mag + 1e-300L); }

// plane kinds: 0 none, 1 all points active, 2 none active, 3 some active (and g = 0 exactly at the first, middle, last point)
static int sweep(int nF, int nJ, int64_t npts, int mask, int kind, double sigma, long *cases) {
  const int64_t nv = (int64_t)nF * nJ * npts, nT = nv * nF * nJ;
  tg_vec_s *u = (mask & 1) ? vec(nv, -1.0, 1.0) : nullptr, *w = (mask & 2) ? vec(nF * npts, -1.0, 1.0) : nullptr;
  tg_vec_s *s = (mask & 4) ? vec(nv, -1.0, 1.0) : nullptr, *T = (mask & 8) ? vec(nT, -1.0, 1.0) : nullptr;
  tg_vec_s *e = (mask & 16) ? vec(npts, 7.0, 7.0) : nullptr, *X0 = kind ? vec(nF * npts, -1.0, 1.0) : nullptr;
  const bool count = mask & 32;
  const double coef[7] = {sigma, 3.25, -1.5, 0.75, 40.0, 20.0, 2.0};
  double plane[5] = {0.6, -0.8, 0.0, 0.0, 0.0};
  if (nF == 3) plane[0] = 0.48, plane[1] = -0.64, plane[2] = 0.6;
  plane[nF] = kind == 1 ? 10.0 : kind == 2 ? -10.0 : 0.125;
  const int64_t zero[3] = {0, npts / 2, npts - 1};
  if (kind == 3)          // g = 0 exactly: X0 = (offset / n_0, 0, ..) - u with exactly representable data (0.125 / 0.6 is not: n_0 -> 0.5)
    for (int64_t q : zero) {
      for (int c = 0; c < nF; c++) {
        X0->d[c * npts + q] = c == 0 ? 0.25 : 0.0;
        if (u) u->d[(int64_t)(c * nJ) * npts + q] = 0.0;
      }
    }
  if (kind == 3) plane[0] = 0.5;       // (the sweep checks addresses and formulas: the normal need not be a unit vector)
  std::vector<double> s0, T0;
  if (s) s0.assign(s->d, s->d + nv);
  if (T) T0.assign(T->d, T->d + nT);
  int64_t nact = -1;
  CHECK(tg_point_dynamics(nF, nJ, npts, coef, kind ? plane : nullptr, X0, u, w, s, T, e, count ? &nact : nullptr));
  int64_t want_active = 0;
  for (int64_t q = 0; q < npts; q++) {
    long double g = 0.0L, gabs = 0.0L;
    if (kind) {
      g = plane[nF], gabs = fabsl(g);
      for (int c = 0; c < nF; c++) {
        const long double xc = (long double)X0->d[c * npts + q] + (u ? (long double)u->d[(int64_t)(c * nJ) * npts + q] : 0.0L);
        g -= plane[c] * xc, gabs += fabsl(plane[c] * xc);
      }
    }
    const bool active = g > 0.0L;
    if (kind == 3 && (q == zero[0] || q == zero[1] || q == zero[2]) && g != 0.0L) return 20;
    want_active += active;
    const long double gp = active ? g : 0.0L;
    long double ww = 0.0L;
    for (int i = 0; i < nF; i++) {
      const long double ui = u ? (long double)u->d[(int64_t)(i * nJ) * npts + q] : 0.0L, wi = w ? (long double)w->d[i * npts + q] : 0.0L;
      ww += wi * wi;
      if (s)
        for (int al = 0; al < nJ; al++) {
          const int64_t at = (int64_t)(i * nJ + al) * npts + q;
          long double want = (long double)sigma * s0[at], mag = fabsl(want);
          if (al == 0) {
            want += coef[1] * ui + coef[2] * wi - coef[4] * gp * plane[i];
            mag += fabsl(coef[1] * ui) + fabsl(coef[2] * wi) + fabsl(coef[4] * plane[i]) * gabs;
          }
          if (!near(s->d[at], want, mag)) return 21;
          if (sigma == 1.0 && al > 0 && memcmp(&s->d[at], &s0[at], sizeof(double))) return 22;
        }
      if (T)
        for (int j = 0; j < nF; j++)
          for (int ab = 0; ab < nJ * nJ; ab++) {
            const int64_t at = (int64_t)((i * nF + j) * nJ * nJ + ab) * npts + q;
            if (ab > 0 || (i != j && !active)) {
              if (memcmp(&T->d[at], &T0[at], sizeof(double))) return 23;
              continue;
            }
            const long double add = (i == j ? (long double)coef[3] : 0.0L) + (active ? (long double)coef[5] * plane[i] * plane[j] : 0.0L);
            if (!near(T->d[at], (long double)T0[at] + add, fabsl(T0[at]) + fabsl(add))) return 24;
          }
    }
    if (e && !near(e->d[q], 0.5L * coef[6] * ww + 0.5L * coef[4] * gp * gp, 1.0L + gabs * gabs * coef[4])) return 25;
  }
  if (count && nact != want_active) return 26;
  if (kind == 1 && want_active != npts) return 27;
  if (kind == 2 && want_active != 0) return 27;
  if (kind == 3 && npts >= 63 && (want_active == 0 || want_active == npts)) return 27;
  if ((s && !finite_all(s->d, nv)) || (T && !finite_all(T->d, nT)) || (e && !finite_all(e->d, npts))) return 2;
  for (tg_vec_s *v : {u, w, s, T, e, X0}) drop(v);
  (*cases)++;
  return 0;
}

int main() {
  g_tg.ready = true;
  g_tg.host_pinned = (double *)malloc(64 * sizeof(double));
  long cases = 0;
  for (const int *sh : kShapes)
    for (int64_t npts : kCounts)
      for (int mask = 0; mask < 64; mask++)
        for (int kind = 0; kind < 4; kind++)
          for (double sigma : {1.0, 1.75})
            if (int rc = sweep(sh[0], sh[1], npts, mask, kind, sigma, &cases)) {
              fprintf(stderr, "point_dynamics_host_sweep: nF = %d, nJ = %d, %lld points, arguments %d, plane kind %d, sigma %g failed "
                      "with %d (%s)\n", sh[0], sh[1], (long long)npts, mask, kind, sigma, rc, g_err);
              return rc;
            }
  // what the driver refuses: other nF and nJ, wrong sizes, a plane without reference positions
  const double coef[7] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, plane[5] = {1.0, 0.0, 0.0, 0.0, 0.0};
  tg_vec_s *a = vec(18, 0.0, 0.0), *b = vec(17, 0.0, 0.0), *x = vec(3, 0.0, 0.0);
  if (tg_point_dynamics(1, 6, 1, coef, nullptr, nullptr, a, nullptr, nullptr, nullptr, nullptr, nullptr) != 2 ||
      tg_point_dynamics(3, 2, 1, coef, nullptr, nullptr, a, nullptr, nullptr, nullptr, nullptr, nullptr) != 2 ||
      tg_point_dynamics(3, 6, 1, nullptr, nullptr, nullptr, a, nullptr, nullptr, nullptr, nullptr, nullptr) != 2 ||
      tg_point_dynamics(3, 6, 1, coef, nullptr, nullptr, b, nullptr, nullptr, nullptr, nullptr, nullptr) != 2 ||
      tg_point_dynamics(3, 6, 1, coef, nullptr, nullptr, a, nullptr, b, nullptr, nullptr, nullptr) != 2 ||
      tg_point_dynamics(3, 6, 1, coef, nullptr, nullptr, a, nullptr, nullptr, a, nullptr, nullptr) != 2 ||
      tg_point_dynamics(3, 6, 1, coef, nullptr, nullptr, a, a, nullptr, nullptr, nullptr, nullptr) != 2 ||
      tg_point_dynamics(3, 6, 1, coef, nullptr, nullptr, a, nullptr, nullptr, nullptr, x, nullptr) != 2 ||
      tg_point_dynamics(3, 6, 1, coef, plane, nullptr, a, nullptr, a, nullptr, nullptr, nullptr) != 2 ||
      tg_point_dynamics(3, 6, 1, coef, plane, a, a, nullptr, a, nullptr, nullptr, nullptr) != 2) {
    fprintf(stderr, "point_dynamics_host_sweep: an argument that should be refused was accepted\n");
    return 13;
  }
  for (tg_vec_s *v : {a, b, x}) drop(v);
  free(g_tg.host_pinned);
  printf("point_dynamics_host_sweep: %ld cases ((nF, nJ) x point counts x optional arguments x planes x sigma), outputs fnv1a "
         "%016llx: clean\n", cases, (unsigned long long)g_fnv);
  return 0;
}
