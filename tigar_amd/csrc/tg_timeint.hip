// Kernels of the time integrators (tigar_amd/timeIntegration.py; tIGAr/timeIntegration.py builds the same formulas
// symbolically in UFL):
//   * tg_vec_lincomb    out = sum_i coef[i] v[i], up to 8 terms in one pass (the alpha-level / predictor expressions)
//   * tg_state_advance  the update of (x_old, xdot_old, xddot_old) at the end of a step, fused and in place
//   * tg_spmv_pair      y = y0 - A xa - B xb for two matrices on ONE sparsity pattern (right-hand side of a step:
//                       f - M w_M - K w_K), 20 B per stored entry instead of 2 x 12 B and one pass over y
// All three are HBM-stream-bound; none uses atomics, so results are bit-reproducible.
#include "tg_common.h"
#include <algorithm>

typedef double tg_d2 __attribute__((ext_vector_type(2)));

#define TG_LINCOMB_MAX 8

struct tg_lin_args {
  const double *v[TG_LINCOMB_MAX];
  double c[TG_LINCOMB_MAX];
};

// Fixed evaluation order (s = c0 v0, then s = fma(ci, vi, s) in index order): the same inputs give the same bits whichever
// of the two variants runs.  `out` may be one of the inputs: a thread reads all inputs of its entries before it writes them,
// and no other thread touches those entries.  VEC: entries in pairs through 16-byte accesses (all pointers 16-byte
// aligned), the odd last entry by one thread.  (tg_grid_1d caps the grid: grid-stride loop, see k_gather_len)
template <bool VEC>
__global__ void __launch_bounds__(256) k_vec_lincomb(tg_lin_args a, int k, double *out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (VEC) {
    const int64_t n2 = n >> 1;
    for (int64_t i = first; i < n2; i += stride) {
      tg_d2 s = a.c[0] * reinterpret_cast<const tg_d2 *>(a.v[0])[i];
#pragma unroll
      for (int j = 1; j < TG_LINCOMB_MAX; j++)
        if (j < k) {
          const tg_d2 w = reinterpret_cast<const tg_d2 *>(a.v[j])[i];
          s.x = fma(a.c[j], w.x, s.x);
          s.y = fma(a.c[j], w.y, s.y);
        }
      reinterpret_cast<tg_d2 *>(out)[i] = s;
    }
    if ((n & 1) && first == 0) {
      double s = a.c[0] * a.v[0][n - 1];
#pragma unroll
      for (int j = 1; j < TG_LINCOMB_MAX; j++)
        if (j < k) s = fma(a.c[j], a.v[j][n - 1], s);
      out[n - 1] = s;
    }
  } else {
    for (int64_t i = first; i < n; i += stride) {
      double s = a.c[0] * a.v[0][i];
#pragma unroll
      for (int j = 1; j < TG_LINCOMB_MAX; j++)
        if (j < k) s = fma(a.c[j], a.v[j][i], s);
      out[i] = s;
    }
  }
}

static inline bool tg_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int tg_vec_lincomb(tg_vec_t out, int k, const double *coef, const tg_vec_t *v) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(out && coef && v, "null argument to tg_vec_lincomb");
  TG_REQUIRE(k >= 1 && k <= TG_LINCOMB_MAX, "tg_vec_lincomb: %d terms (1 to %d are taken in one pass)", k, TG_LINCOMB_MAX);
  tg_lin_args a;
  bool vec = tg_aligned16(out->d);
  for (int j = 0; j < TG_LINCOMB_MAX; j++) {
    a.v[j] = nullptr;
    a.c[j] = 0.0;
  }
  for (int j = 0; j < k; j++) {
    TG_REQUIRE(v[j], "tg_vec_lincomb: term %d is a null vector", j);
    TG_REQUIRE(v[j]->n == out->n, "tg_vec_lincomb: term %d has %lld entries, the result %lld", j, (long long)v[j]->n,
               (long long)out->n);
    a.v[j] = v[j]->d;
    a.c[j] = coef[j];
    vec = vec && tg_aligned16(v[j]->d);
  }
  const int64_t n = out->n;
  if (n == 0) return 0;
  if (vec)
    hipLaunchKernelGGL((k_vec_lincomb<true>), dim3(tg_grid_1d((n + 1) / 2, 256)), dim3(256), 0, g_tg.stream, a, k, out->d, n);
  else
    hipLaunchKernelGGL((k_vec_lincomb<false>), dim3(tg_grid_1d(n, 256)), dim3(256), 0, g_tg.stream, a, k, out->d, n);
  TG_LAUNCH_CHECK();
  return 0;
}

// ---- state update of a time step --------------------------------------------------------------------------------------
//   v = c0 x + c1 x_old + c2 xdot_old + c3 xddot_old,  a = c4 v + c5 xdot_old + c6 xddot_old,
//   x_old = x, xdot_old = v, xddot_old = a
// An entry's four values sit in registers before any of them is overwritten, so the copies with which
// tIGAr/timeIntegration.py:228-247 avoids reading updated values are not needed.  SECOND = false: no acceleration vector
// (c3 and the `a` line are ignored).  Reads 4 (3) vectors, writes 3 (2).
struct tg_adv_coef {
  double c[7];
};

template <bool SECOND>
__device__ __forceinline__ void tg_advance_entry(const tg_adv_coef &c, double x, double &xo, double &vo, double &ao) {
  double v = c.c[0] * x;
  v = fma(c.c[1], xo, v);
  v = fma(c.c[2], vo, v);
  if (SECOND) {
    v = fma(c.c[3], ao, v);
    double a = c.c[4] * v;
    a = fma(c.c[5], vo, a);
    a = fma(c.c[6], ao, a);
    ao = a;
  }
  xo = x;
  vo = v;
}

template <bool SECOND, bool VEC>
__global__ void __launch_bounds__(256)
    k_state_advance(tg_adv_coef c, const double *x, double *x_old, double *xdot_old, double *xddot_old, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (VEC) {
    const int64_t n2 = n >> 1;
    for (int64_t i = first; i < n2; i += stride) {
      const tg_d2 xx = reinterpret_cast<const tg_d2 *>(x)[i];
      const tg_d2 xo = reinterpret_cast<const tg_d2 *>(x_old)[i];
      const tg_d2 vo = reinterpret_cast<const tg_d2 *>(xdot_old)[i];
      tg_d2 ao = {0.0, 0.0};
      if (SECOND) ao = reinterpret_cast<const tg_d2 *>(xddot_old)[i];
      double xo0 = xo.x, xo1 = xo.y, vo0 = vo.x, vo1 = vo.y, ao0 = ao.x, ao1 = ao.y;
      tg_advance_entry<SECOND>(c, xx.x, xo0, vo0, ao0);
      tg_advance_entry<SECOND>(c, xx.y, xo1, vo1, ao1);
      reinterpret_cast<tg_d2 *>(x_old)[i] = tg_d2{xo0, xo1};
      reinterpret_cast<tg_d2 *>(xdot_old)[i] = tg_d2{vo0, vo1};
      if (SECOND) reinterpret_cast<tg_d2 *>(xddot_old)[i] = tg_d2{ao0, ao1};
    }
  }
  // scalar entries: all of them, or the odd last one
  for (int64_t i = (VEC ? (n & ~1ll) : 0) + first; i < n; i += stride) {
    double xo = x_old[i], vo = xdot_old[i], ao = SECOND ? xddot_old[i] : 0.0;
    tg_advance_entry<SECOND>(c, x[i], xo, vo, ao);
    x_old[i] = xo;
    xdot_old[i] = vo;
    if (SECOND) xddot_old[i] = ao;
  }
}

extern "C" int tg_state_advance(int order, const double *c, tg_vec_t x, tg_vec_t x_old, tg_vec_t xdot_old, tg_vec_t xddot_old) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(order == 1 || order == 2, "tg_state_advance: order %d (1 or 2)", order);
  TG_REQUIRE(c && x && x_old && xdot_old, "null argument to tg_state_advance");
  TG_REQUIRE((order == 2) == (xddot_old != nullptr), "tg_state_advance: order 2 takes an acceleration vector, order 1 none");
  TG_REQUIRE(x_old->n == x->n && xdot_old->n == x->n && (!xddot_old || xddot_old->n == x->n),
             "tg_state_advance: the vectors differ in size");
  const tg_vec_t vs[4] = {x, x_old, xdot_old, xddot_old};
  for (int i = 0; i < 4; i++)
    for (int j = i + 1; j < 4; j++)
      TG_REQUIRE(!vs[j] || (vs[i] != vs[j] && (vs[i]->d != vs[j]->d || x->n == 0)),
                 "tg_state_advance: x, x_old, xdot_old and xddot_old must be distinct vectors");
  const int64_t n = x->n;
  if (n == 0) return 0;
  tg_adv_coef cc;
  for (int i = 0; i < 7; i++) cc.c[i] = c[i];
  const bool vec = tg_aligned16(x->d) && tg_aligned16(x_old->d) && tg_aligned16(xdot_old->d) &&
                   (!xddot_old || tg_aligned16(xddot_old->d));
  const dim3 grid(tg_grid_1d(vec ? (n + 1) / 2 : n, 256));
  double *ao = xddot_old ? xddot_old->d : nullptr;
#define TG_ADVANCE(SECOND, VEC) \
  hipLaunchKernelGGL((k_state_advance<SECOND, VEC>), grid, dim3(256), 0, g_tg.stream, cc, x->d, x_old->d, xdot_old->d, ao, n)
  if (order == 2) {
    if (vec) TG_ADVANCE(true, true);
    else TG_ADVANCE(true, false);
  } else {
    if (vec) TG_ADVANCE(false, true);
    else TG_ADVANCE(false, false);
  }
#undef TG_ADVANCE
  TG_LAUNCH_CHECK();
  return 0;
}

// ---- y = y0 - A xa - B xb on one pattern -------------------------------------------------------------------------------
struct tg_csr_pair_s {
  tg_csr_s *a = nullptr, *b = nullptr;   // borrowed: the pair does not own them
};

template <typename T>
__global__ void k_pair_equal(int64_t n, const T *__restrict__ a, const T *__restrict__ b, int *__restrict__ mismatch) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (; q < n; q += stride) bad |= (a[q] != b[q]);
  if (bad) atomicOr(mismatch, 1);
}

extern "C" int tg_csr_pair_create(tg_csr_t A, tg_csr_t B, tg_csr_pair_t *out) {
  TG_REQUIRE_CANONICAL(A);
  TG_REQUIRE_CANONICAL(B);
  TG_REQUIRE_INIT();
  TG_REQUIRE(A && B && out, "bad arguments to tg_csr_pair_create");
  TG_REQUIRE(A->nrows == B->nrows && A->ncols == B->ncols && A->nnz == B->nnz,
             "tg_csr_pair_create: the operands differ in shape or nnz");
  int *flag = (int *)g_tg.scratch;
  TG_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int), g_tg.stream));
  if (A != B) {
    hipLaunchKernelGGL((k_pair_equal<int64_t>), dim3(tg_grid_1d(A->nrows + 1, 256)), dim3(256), 0, g_tg.stream, A->nrows + 1,
                       A->rowptr, B->rowptr, flag);
    if (A->nnz > 0)
      hipLaunchKernelGGL((k_pair_equal<int32_t>), dim3(tg_grid_1d(A->nnz, 256)), dim3(256), 0, g_tg.stream, A->nnz, A->col,
                         B->col, flag);
  }
  int h = 0;
  TG_CHECK_HIP(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, g_tg.stream));
  if (hipStreamSynchronize(g_tg.stream) != hipSuccess || hipGetLastError() != hipSuccess) {
    tg_set_error("tg_csr_pair_create: kernel failed");
    return 1;
  }
  if (h) {
    tg_set_error("tg_csr_pair_create: the operands do not share one sparsity pattern");
    return 2;
  }
  tg_csr_pair_s *p = new tg_csr_pair_s();
  p->a = A;
  p->b = B;
  *out = p;
  return 0;
}

extern "C" int tg_csr_pair_destroy(tg_csr_pair_t p) {
  delete p;
  return 0;
}

// k_spmv_lane (tg_sparse.hip) for two value arrays: A's row blocks, lane-major entry mapping, each entry's column loaded
// ONCE for both gathers, the sum of the two products parked in the LDS slot, the same row reduction, y0 added in its
// last line.  The slices of a block go through the registers in chunks of at most 16 (4096 entries: two values, a column
// and two gathered operands per slice and lane stay well inside the register file of a 256-thread workgroup).
// y may alias y0 (the lane that writes y[r] has read y0[r]); it must not alias xa or xb.
template <int CAP>
__global__ void __launch_bounds__(256)
    k_spmv_pair_lane(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ va,
                     const double *__restrict__ vb, const double *__restrict__ xa, const double *__restrict__ xb,
                     const double *y0, double *y, const int32_t *__restrict__ rowblocks, int64_t nblocks) {
  __shared__ double prod[CAP];
  const int tid = threadIdx.x;
  const int64_t L = tg_xcd_block(blockIdx.x, nblocks);
  if (L >= nblocks) return;
  const int64_t r0 = rowblocks[L], r1 = rowblocks[L + 1];
  if (r1 <= r0) return;
  const int64_t n0 = rowptr[r0], n1 = rowptr[r1];
  if (n1 <= n0) {                                  // a block of empty rows: see k_spmv_stream
    for (int64_t r = r0 + tid; r < r1; r += 256) y[r] = y0 ? y0[r] : 0.0;
    return;
  }
  constexpr int SL = CAP / 256;
  constexpr int CH = SL < 16 ? SL : 16;
#pragma unroll
  for (int k0 = 0; k0 < SL; k0 += CH) {
    if (n0 + 256 * k0 >= n1) break;                // (uniform over the workgroup)
    double a[CH], b[CH];
    int32_t c[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) {
      int64_t t = n0 + tid + 256 * (k0 + k);
      t = t < n1 ? t : n1 - 1;
      a[k] = va[t];
      b[k] = vb[t];
      c[k] = col[t];
    }
    double ga[CH], gb[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) {
      ga[k] = xa[c[k]];
      gb[k] = xb[c[k]];
    }
#pragma unroll
    for (int k = 0; k < CH; k++) {
      const int64_t t = n0 + tid + 256 * (k0 + k);
      if (t < n1) prod[t - n0] = a[k] * ga[k] + b[k] * gb[k];
    }
  }
  __syncthreads();
  const int nr = (int)(r1 - r0);
  int G = 1;
  while (G < 64 && G * 2 * nr <= 256) G <<= 1;
  const int rows_per_pass = 256 / G;
  const int sub = tid & (G - 1);
  const int rgrp = tid / G;
  for (int base = 0; base < nr; base += rows_per_pass) {
    const int rr = base + rgrp;
    double s = 0.0;
    if (rr < nr) {
      const int64_t p = rowptr[r0 + rr] - n0, q1 = rowptr[r0 + rr + 1] - n0;
      for (int64_t q = p + sub; q < q1; q += G) s += prod[q];
    }
    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (rr < nr && sub == 0) y[r0 + rr] = (y0 ? y0[r0 + rr] : 0.0) - s;
  }
}

// one wave per row (a row longer than half the largest LDS stage: the plan's wave-per-row mode), as k_spmv_vector
__global__ void __launch_bounds__(256)
    k_spmv_pair_vector(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ va,
                       const double *__restrict__ vb, const double *__restrict__ xa, const double *__restrict__ xb,
                       const double *y0, double *y, int64_t nrows) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < nrows; r += nwaves) {
    double s = 0.0;
    for (int64_t q = rowptr[r] + lane; q < rowptr[r + 1]; q += 64) {
      const int32_t c = col[q];
      s += va[q] * xa[c] + vb[q] * xb[c];
    }
    s = tg_wave_sum(s);
    if (lane == 0) y[r] = (y0 ? y0[r] : 0.0) - s;
  }
}

extern "C" int tg_spmv_pair(tg_csr_pair_t p, tg_vec_t xa, tg_vec_t xb, tg_vec_t y0, tg_vec_t y) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(p && xa && xb && y, "null argument to tg_spmv_pair");
  tg_csr_s *a = p->a, *b = p->b;
  TG_REQUIRE(a->nrows == b->nrows && a->ncols == b->ncols && a->nnz == b->nnz,
             "tg_spmv_pair: a matrix of the pair changed shape after tg_csr_pair_create");
  TG_REQUIRE(xa->n == a->ncols && xb->n == a->ncols, "tg_spmv_pair: operands of %lld and %lld entries, the matrices have %lld columns",
             (long long)xa->n, (long long)xb->n, (long long)a->ncols);
  TG_REQUIRE(y->n == a->nrows && (!y0 || y0->n == a->nrows), "tg_spmv_pair: y (and y0) must have %lld entries", (long long)a->nrows);
  TG_REQUIRE(y != xa && y != xb && (y->n == 0 || (y->d != xa->d && y->d != xb->d)), "tg_spmv_pair: y must differ from xa and xb");
  TG_TRY(tg_spmv_plan(a));
  if (a->nrows == 0) return 0;
  const double *y0d = y0 ? y0->d : nullptr;
  if (a->spmv_mode == 1) {
    const unsigned grid = (unsigned)(((a->nblocks + 7) / 8) * 8);  // tg_xcd_block needs a multiple of 8
#define TG_SPMV_PAIR(CAP)                                                                                              \
  hipLaunchKernelGGL((k_spmv_pair_lane<CAP>), dim3(grid), dim3(256), 0, g_tg.stream, a->rowptr, a->col, a->val, b->val, \
                     xa->d, xb->d, y0d, y->d, a->rowblocks, a->nblocks)
    if (a->spmv_cap == 1024) TG_SPMV_PAIR(1024);
    else if (a->spmv_cap == 2048) TG_SPMV_PAIR(2048);
    else if (a->spmv_cap == 4096) TG_SPMV_PAIR(4096);
    else TG_SPMV_PAIR(8192);
#undef TG_SPMV_PAIR
  } else {
    const unsigned grid = (unsigned)std::min<int64_t>(tg_cdiv(a->nrows, 4), (int64_t)g_tg.num_cu * 8);
    hipLaunchKernelGGL(k_spmv_pair_vector, dim3(grid), dim3(256), 0, g_tg.stream, a->rowptr, a->col, a->val, b->val, xa->d,
                       xb->d, y0d, y->d, a->nrows);
  }
  TG_LAUNCH_CHECK();
  return 0;
}
