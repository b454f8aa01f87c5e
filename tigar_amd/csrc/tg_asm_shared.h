// What the element kernels on mapped patches share (tg_assemble.hip: the forms; tg_postproc.hip: quadrature-point
// evaluation, loads from point values, error norms): limits, the inverse of the metric, and the device copies of the
// element vertices and of the reference-element tables l[a][q] | dl[a][q] | w[q] | d2l[a][q].
#pragma once
#include "tg_common.h"

#define TG_ASM_MAXLOC 128      // (p+1)^d local nodes: p <= 4 in 3-D, p <= 8 in 2-D (<= 81), any p <= 8 in 1-D
#define TG_ASM_MAXQ1 10        // Gauss points per direction
#define TG_SYSTEM_MAX_FIELDS 16   // fields of a first-order system (tg_coef_transform_system; tg_csr_from_blocks takes 16)

__device__ __forceinline__ void tg_sym_inverse(int d, const double *g, double *gi, double *det) {
  if (d == 1) {
    *det = g[0];
    gi[0] = 1.0 / g[0];
  } else if (d == 2) {
    const double a = g[0], b = g[1], c = g[3];
    const double dt = a * c - b * b;
    *det = dt;
    gi[0] = c / dt;
    gi[1] = gi[2] = -b / dt;
    gi[3] = a / dt;
  } else {
    const double a = g[0], b = g[1], c = g[2], e = g[4], f = g[5], i = g[8];
    const double c00 = e * i - f * f, c01 = c * f - b * i, c02 = b * f - c * e;
    const double dt = a * c00 + b * c01 + c * c02;
    *det = dt;
    gi[0] = c00 / dt;
    gi[1] = gi[3] = c01 / dt;
    gi[2] = gi[6] = c02 / dt;
    gi[4] = (a * i - c * c) / dt;
    gi[5] = gi[7] = (b * c - a * f) / dt;
    gi[8] = (a * e - b * b) / dt;
  }
}

struct tg_asm_cache_t {
  int d = 0, p = 0, nq = 0, nverts[3] = {0, 0, 0};
  std::vector<double> hverts[3];
  double *verts[3] = {nullptr, nullptr, nullptr};
  double *tab = nullptr;
};
extern tg_asm_cache_t g_asm_cache;
int tg_asm_cache_get(const tg_patch_t *pt);   // uploads (or keeps) the tables of this patch description
// the element-coupling pattern with its certificate, rows [row0, row1); n[k] nodes per direction (tg_assemble.hip)
int tg_asm_coupling_pattern(int d, int p, const int *n, int64_t row0, int64_t row1, bool pattern_only, tg_csr_t *out);
// the point-coefficient form of tg_coef.hip through the sum-factorised kernels, where the shape has such a route (*taken)
int tg_asm_coef_fast(const tg_patch_t *pt, tg_vec_t coef, tg_csr_t *out, bool *taken);
