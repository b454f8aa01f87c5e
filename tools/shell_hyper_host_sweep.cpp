// Sanitizer sweep of the hyperelastic Kirchhoff-Love law (kind 1 of tg_shell_points) and of the follower-pressure kernel
// (tg_shell_pressure_points) on the CPU: the kernel source of csrc/tg_shell.hip WITH its host drivers, compiled as plain C++
// against tools/host_shim and run block by block with every array allocated at exactly its size.  Sweeps n_thickness = 1..4,
// point counts around the workgroup size, every subset of outputs, and inadmissible points -- coincident current tangents and a
// curvature that turns det C_2D negative -- at the first, middle and last point.  Build and run (no GPU, no Python):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -x c++ \
//           -Itools/host_shim -Iinclude tools/shell_hyper_host_sweep.cpp -o shell_hyper_host_sweep && ./shell_hyper_host_sweep
//
// Besides addresses it checks what costs nothing here (loose bounds; tests/test_gpu_shell_hyper.py holds the figures): the law
// against central differences of its own energy and load, the major symmetry of its tangent, the pressure tangent against
// central differences of the pressure load, that a subset of outputs has the bits of the full call, and that inadmissible
// points are counted and their outputs left alone.
#define TG_HOST_SWEEP_JET
#include "host_shim/tg_host_sweep.h"

static const int64_t kCounts[] = {1, 63, 255, 256, 257, 1000};

// a surface close to the plane with curvature: X_,0 ~ e_0, X_,1 ~ 1.2 e_1
static void make_jets(int64_t npts, tg_vec_s **X, tg_vec_s **U) {
  *X = vec(18 * npts, -0.15, 0.15), *U = vec(18 * npts, -0.05, 0.05);
  for (int64_t q = 0; q < npts; q++) {
    (*X)->d[(6 * 0 + 1) * npts + q] += 1.0;
    (*X)->d[(6 * 1 + 2) * npts + q] += 1.2;
  }
}

static bool same_bits(const tg_vec_s *a, const tg_vec_s *b) { return memcmp(a->d, b->d, a->n * sizeof(double)) == 0; }

static int sweep_law(int nth, long *cases) {
  const double par[3] = {1.0e3, 0.3, (double)nth};
  for (int64_t npts : kCounts) {
    tg_vec_s *X, *U;
    make_jets(npts, &X, &U);
    tg_vec_s *sf = vec(18 * npts, 0.0, 0.0), *Tf = vec(324 * npts, 0.0, 0.0), *pf = vec(npts, 0.0, 0.0);
    int64_t nbad = -1;
    CHECK(tg_shell_points(1, par, npts, X, U, sf, Tf, pf, &nbad));
    if (nbad != 0) return 3;
    for (int mask = 0; mask < 8; mask++) {
      tg_vec_s *s = (mask & 1) ? vec(18 * npts, 0.0, 0.0) : nullptr, *T = (mask & 2) ? vec(324 * npts, 0.0, 0.0) : nullptr;
      tg_vec_s *psi = (mask & 4) ? vec(npts, 0.0, 0.0) : nullptr;
      nbad = -1;
      CHECK(tg_shell_points(1, par, npts, X, U, s, T, psi, &nbad));
      if (nbad != 0) return 3;
      if ((s && !finite_all(s->d, s->n)) || (T && !finite_all(T->d, T->n)) || (psi && !finite_all(psi->d, psi->n))) return 2;
      if ((s && !same_bits(s, sf)) || (T && !same_bits(T, Tf)) || (psi && !same_bits(psi, pf))) return 10;
      for (tg_vec_s *v : {s, T, psi}) drop(v);
      (*cases)++;
    }
    // central differences at the first point: d psi / d jet = s, d s / d jet = T
    const double h = 1e-5;
    for (int j = 0; j < 3; j++)
      for (int be = 0; be < 6; be++) {
        tg_vec_s *sp = vec(18 * npts, 0.0, 0.0), *sm = vec(18 * npts, 0.0, 0.0), *pp = vec(npts, 0.0, 0.0), *pm = vec(npts, 0.0, 0.0);
        double &x = U->d[(6 * j + be) * npts], x0 = x;
        x = x0 + h;
        CHECK(tg_shell_points(1, par, npts, X, U, sp, nullptr, pp, &nbad));
        x = x0 - h;
        CHECK(tg_shell_points(1, par, npts, X, U, sm, nullptr, pm, &nbad));
        x = x0;
        const double scale = 1.0 + fabs(sf->d[(6 * j + be) * npts]);
        if (fabs((pp->d[0] - pm->d[0]) / (2 * h) - sf->d[(6 * j + be) * npts]) > 1e-5 * scale) return 4;
        for (int i = 0; i < 3; i++)
          for (int al = 0; al < 6; al++) {
            const double t = Tf->d[((3 * i + j) * 36 + 6 * al + be) * npts];
            if (fabs((sp->d[(6 * i + al) * npts] - sm->d[(6 * i + al) * npts]) / (2 * h) - t) > 1e-5 * (1.0 + fabs(t)) * 10) return 5;
            if (fabs(t - Tf->d[((3 * j + i) * 36 + 6 * be + al) * npts]) > 1e-10 * (1.0 + fabs(t))) return 8;
          }
        for (tg_vec_s *v : {sp, sm, pp, pm}) drop(v);
      }
    for (tg_vec_s *v : {sf, Tf, pf}) drop(v);
    // inadmissible points at the first, middle and last point, of two kinds: counted, their outputs left alone
    for (int how = 0; how < 2; how++) {
      tg_vec_s *X2, *U2;
      make_jets(npts, &X2, &U2);
      const int64_t bad[3] = {0, npts / 2, npts - 1};
      int64_t nb = 0;
      for (int b = 0; b < 3; b++) {
        bool seen = false;
        for (int c = 0; c < b; c++) seen = seen || bad[c] == bad[b];
        if (seen) continue;
        nb++;
        const int64_t q = bad[b];
        if (how == 0) {
          for (int c = 0; c < 3; c++)              // x_,1 = x_,0: the current normal vanishes
            U2->d[(6 * c + 2) * npts + q] = X2->d[(6 * c + 1) * npts + q] + U2->d[(6 * c + 1) * npts + q] - X2->d[(6 * c + 2) * npts + q];
        } else {                                   // u_,00 += 40 a_3: gm_00 = a_00 - 2 xi b_00 < 0 at every xi > 0.0125 a_00
          double g[2][3], n[3];
          for (int a = 0; a < 2; a++)
            for (int c = 0; c < 3; c++) g[a][c] = X2->d[(6 * c + 1 + a) * npts + q] + U2->d[(6 * c + 1 + a) * npts + q];
          tg_shell_cross(g[0], g[1], n);
          const double nn = sqrt(tg_shell_dot(n, n));
          for (int c = 0; c < 3; c++) U2->d[(6 * c + 3) * npts + q] += 40.0 * n[c] / nn;
        }
      }
      tg_vec_s *s = vec(18 * npts, 0.0, 0.0), *T = vec(324 * npts, 0.0, 0.0), *psi = vec(npts, 0.0, 0.0);
      CHECK(tg_shell_points(1, par, npts, X2, U2, s, T, psi, &nbad));
      // (one thickness point sits on the midsurface, where the curvature does not enter: how = 1 is admissible for nth = 1)
      if (nbad != (how == 1 && nth == 1 ? 0 : nb)) return 6;
      if (nbad && (psi->d[bad[0]] != 0.0 || s->d[npts + bad[0]] != 0.0 || T->d[7 * npts + bad[0]] != 0.0)) return 7;   // (as vec() left them)
      for (tg_vec_s *v : {s, T, psi, X2, U2}) drop(v);
      (*cases)++;
    }
    drop(X), drop(U);
  }
  return 0;
}

static int sweep_pressure(long *cases) {
  const double P = 7.0;
  for (int64_t npts : kCounts) {
    tg_vec_s *X, *U;
    make_jets(npts, &X, &U);
    // a degenerate reference normal at the last point: left alone
    for (int c = 0; c < 3; c++) X->d[(6 * c + 2) * npts + npts - 1] = X->d[(6 * c + 1) * npts + npts - 1];
    for (int mask = 0; mask < 4; mask++) {
      tg_vec_s *s = (mask & 1) ? vec(18 * npts, 1.0, 1.0) : nullptr, *T = (mask & 2) ? vec(324 * npts, 1.0, 1.0) : nullptr;
      CHECK(tg_shell_pressure_points(npts, P, X, U, s, T));
      if ((s && !finite_all(s->d, s->n)) || (T && !finite_all(T->d, T->n))) return 2;
      if (s && (s->d[npts - 1] != 1.0 || s->d[npts + 0] != 1.0)) return 11;          // the degenerate point; a derivative slot
      if (T && (T->d[npts + npts - 1] != 1.0 || T->d[0] != 1.0)) return 11;          // the degenerate point; the (0, 0) entry
      for (tg_vec_s *v : {s, T}) drop(v);
      (*cases)++;
    }
    // the tangent against central differences of the load at the first point (npts > 1: the last point is degenerate)
    if (npts > 1) {
      tg_vec_s *s = vec(18 * npts, 0.0, 0.0), *T = vec(324 * npts, 0.0, 0.0);
      CHECK(tg_shell_pressure_points(npts, P, X, U, s, T));
      const double h = 1e-5;
      for (int j = 0; j < 3; j++)
        for (int be = 0; be < 6; be++) {
          tg_vec_s *sp = vec(18 * npts, 0.0, 0.0), *sm = vec(18 * npts, 0.0, 0.0);
          double &x = U->d[(6 * j + be) * npts], x0 = x;
          x = x0 + h;
          CHECK(tg_shell_pressure_points(npts, P, X, U, sp, nullptr));
          x = x0 - h;
          CHECK(tg_shell_pressure_points(npts, P, X, U, sm, nullptr));
          x = x0;
          for (int i = 0; i < 3; i++)
            for (int al = 0; al < 6; al++) {
              const double t = T->d[((3 * i + j) * 36 + 6 * al + be) * npts];
              if (fabs((sp->d[(6 * i + al) * npts] - sm->d[(6 * i + al) * npts]) / (2 * h) - t) > 1e-6 * (1.0 + fabs(t))) return 12;
            }
          drop(sp), drop(sm);
        }
      drop(s), drop(T);
      (*cases)++;
    }
    drop(X), drop(U);
  }
  return 0;
}

int main() {
  g_tg.ready = true;
  g_tg.host_pinned = (double *)malloc(64 * sizeof(double));
  long cases = 0;
  for (int nth = 1; nth <= 4; nth++)
    if (int rc = sweep_law(nth, &cases)) {
      fprintf(stderr, "shell_hyper_host_sweep: the law with %d thickness points failed with %d (%s)\n", nth, rc, g_err);
      return rc;
    }
  if (int rc = sweep_pressure(&cases)) {
    fprintf(stderr, "shell_hyper_host_sweep: the pressure kernel failed with %d (%s)\n", rc, g_err);
    return rc;
  }
  // what the driver refuses
  const double bad_par[3] = {1.0, 0.1, 5.0};
  tg_vec_s *X = vec(18, 0.0, 0.0), *U = vec(18, 0.0, 0.0);
  int64_t nbad;
  if (tg_shell_points(1, bad_par, 1, X, U, nullptr, nullptr, nullptr, &nbad) == 0 ||
      tg_shell_points(2, bad_par, 1, X, U, nullptr, nullptr, nullptr, &nbad) == 0) {
    fprintf(stderr, "shell_hyper_host_sweep: five thickness points or kind 2 were not refused\n");
    return 13;
  }
  drop(X), drop(U);
  free(g_tg.host_pinned);
  printf("shell_hyper_host_sweep: %ld cases (law: thickness points x point counts x (outputs + inadmissible kinds); pressure: point "
         "counts x outputs + differences), outputs fnv1a %016llx: clean\n", cases, (unsigned long long)g_fnv);
  return 0;
}
