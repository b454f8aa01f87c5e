// Block kernels of the LOBPCG eigensolver (tigar_amd/eigen.py).
//
// A block is a tg_vec_t of n*k doubles, row-major: entry (i, j) at i*k + j, 1 <= k <= TG_BLOCK_MAX.  Every kernel writes its
// results with plain stores, uses no floating-point atomics and sums in an order fixed by the shapes alone, so each result
// is the same bits from run to run.
//
//   tg_spmm                 Y = A X, one wave per row of A: the wave reads 64 entries of the row at a time (coalesced), lane
//                           groups of the next power of two >= k take them in turn through shuffles (unrolled: the gathers
//                           of X for the 64 entries are issued together), a shuffle tree adds the groups.  A is read once
//                           whatever k.
//   tg_block_gram           G = X^T Y: per workgroup a fixed chunk of rows staged in LDS, partial Gram matrices to a
//                           buffer, a second pass adds them in block order, result to the host.
//   tg_block_combine        Y = sum_s X_s C_s (s < 3), C_s small host matrices.
//   tg_block_residual       R = AX - BX diag(lam), masked rows zeroed, optional W = D^-1 R, per-column |R_j|^2 and |BX_j|^2.
//   tg_block_get/set_column column j <-> a plain vector.
//   tg_csr_decoupled_rows   rows whose only non-zero is the diagonal, in A and in B (zero dofs of extractMatrix), + diagonals
//                           and the largest sum |a_ij| over the other rows.
//   tg_csr_sym_defect       max |A_ij - A_ji| (A against its explicit transpose) and max |A_ij| over i != j.
#include "tg_common.h"

#define TG_BLOCK_MAX 64
#define TG_GRAM_TILE 32                        // rows of X and Y staged per LDS tile
#define TG_GRAM_PER_THREAD (TG_BLOCK_MAX * TG_BLOCK_MAX / 256)
#define TG_BLOCK_PARTS 512                     // most workgroups of the two-pass reductions

#define TG_REQUIRE_WIDTH(k) \
  TG_REQUIRE((k) >= 1 && (k) <= TG_BLOCK_MAX, "%s: block width %d outside [1, %d]", __func__, (int)(k), TG_BLOCK_MAX)

// pinned host staging of the small results (Gram matrices, column norms): a device-to-host copy into pageable memory costs
// a staged transfer each time
#define TG_EIG_PINNED (TG_BLOCK_MAX * TG_BLOCK_MAX)
static double *g_eig_pinned = nullptr;
static int tg_eig_pinned(double **p) {
  if (!g_eig_pinned) TG_CHECK_HIP(hipHostMalloc((void **)&g_eig_pinned, TG_EIG_PINNED * sizeof(double), hipHostMallocDefault));
  *p = g_eig_pinned;
  return 0;
}

// rows per workgroup of the two-pass reductions: at least `min_rows`, at most TG_BLOCK_PARTS workgroups
static inline void tg_block_parts(int64_t n, int64_t min_rows, int64_t *chunk, int *nparts) {
  int64_t c = std::max<int64_t>(min_rows, tg_cdiv(n, TG_BLOCK_PARTS));
  *chunk = c;
  *nparts = (int)std::max<int64_t>(1, tg_cdiv(n, c));
}

// ------------------------------------------------------------------------------------------------- SpMM
template <int KP>
__global__ void __launch_bounds__(256)
    k_spmm(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ val,
           const double *__restrict__ X, double *__restrict__ Y, int64_t nrows, int k) {
  constexpr int G = 64 / KP;                 // lane groups; lane = g * KP + j
  const int lane = threadIdx.x & 63;
  const int g = lane / KP, j = lane % KP;
  const bool jok = j < k;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < nrows; r += nwaves) {
    const int64_t s = rowptr[r], e = rowptr[r + 1];
    double acc = 0.0;
    for (int64_t base = s; base < e; base += 64) {
      const int64_t q = base + lane;
      const int cnt = (int)std::min<int64_t>(64, e - base);
      const int32_t c = q < e ? col[q] : 0;
      const double v = q < e ? val[q] : 0.0;
      // KP steps of G entries per chunk, in batches of U unrolled steps: the gathers of X of a batch are in flight at once
      constexpr int U = KP < 8 ? KP : 8;
      for (int t0 = 0; t0 < cnt; t0 += U * G) {
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int src = t0 + u * G + g;      // entry base + src of the row goes to group g
          const int32_t cc = __shfl(c, src, 64);
          const double vv = __shfl(v, src, 64);
          const double xv = (src < cnt && jok) ? X[(int64_t)cc * k + j] : 0.0;
          acc += vv * xv;                      // (vv = xv = 0 past the end of the row: adds +0)
        }
      }
    }
#pragma unroll
    for (int o = 32; o >= KP; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (g == 0 && jok) Y[r * k + j] = acc;
  }
}

extern "C" int tg_spmm(tg_csr_t a, tg_vec_t x, int k, tg_vec_t y) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(a && x && y, "tg_spmm: null argument");
  TG_REQUIRE_WIDTH(k);
  TG_REQUIRE(!a->rowcnt && !a->view && !a->rowptr_val,
             "tg_spmm: loose-row or view CSR (an intermediate of a PtAP stage); call tg_csr_compact first");
  TG_REQUIRE(x->n == a->ncols * k, "tg_spmm: X has %lld entries, expected %lld columns x %d", (long long)x->n,
             (long long)a->ncols, k);
  TG_REQUIRE(y->n == a->nrows * k, "tg_spmm: Y has %lld entries, expected %lld rows x %d", (long long)y->n,
             (long long)a->nrows, k);
  TG_REQUIRE(x->d != y->d || a->nrows == 0, "tg_spmm: X and Y must be different blocks");
  if (a->nrows == 0) return 0;
  const unsigned grid = (unsigned)std::min<int64_t>(tg_cdiv(a->nrows, 4), (int64_t)g_tg.num_cu * 16);
#define TG_SPMM(KP)                                                                                            \
  hipLaunchKernelGGL((k_spmm<KP>), dim3(grid), dim3(256), 0, g_tg.stream, a->rowptr, a->col, a->val, x->d, y->d, \
                     a->nrows, k)
  if (k <= 1) TG_SPMM(1);
  else if (k <= 2) TG_SPMM(2);
  else if (k <= 4) TG_SPMM(4);
  else if (k <= 8) TG_SPMM(8);
  else if (k <= 16) TG_SPMM(16);
  else if (k <= 32) TG_SPMM(32);
  else TG_SPMM(64);
#undef TG_SPMM
  TG_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------- Gram
__global__ void __launch_bounds__(256)
    k_block_gram(const double *__restrict__ X, int kx, const double *__restrict__ Y, int ky, int64_t n, int64_t chunk,
                 double *__restrict__ partial) {
  __shared__ double xs[TG_GRAM_TILE * TG_BLOCK_MAX], ys[TG_GRAM_TILE * TG_BLOCK_MAX];
  const int t = threadIdx.x;
  const int ne = kx * ky;
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = std::min<int64_t>(n, r0 + chunk);
  double acc[TG_GRAM_PER_THREAD];
  int ia[TG_GRAM_PER_THREAD], ib[TG_GRAM_PER_THREAD];
#pragma unroll
  for (int s = 0; s < TG_GRAM_PER_THREAD; s++) {
    const int e = t + 256 * s;
    acc[s] = 0.0;
    ia[s] = e < ne ? e / ky : 0;
    ib[s] = e < ne ? e - (e / ky) * ky : 0;
  }
  for (int64_t tr = r0; tr < r1; tr += TG_GRAM_TILE) {
    const int rows = (int)std::min<int64_t>(TG_GRAM_TILE, r1 - tr);
    for (int i = t; i < rows * kx; i += 256) xs[i] = X[tr * kx + i];
    for (int i = t; i < rows * ky; i += 256) ys[i] = Y[tr * ky + i];
    __syncthreads();
    for (int r = 0; r < rows; r++) {
#pragma unroll
      for (int s = 0; s < TG_GRAM_PER_THREAD; s++)
        if (t + 256 * s < ne) acc[s] += xs[r * kx + ia[s]] * ys[r * ky + ib[s]];
    }
    __syncthreads();
  }
#pragma unroll
  for (int s = 0; s < TG_GRAM_PER_THREAD; s++)
    if (t + 256 * s < ne) partial[(int64_t)blockIdx.x * ne + t + 256 * s] = acc[s];
}

// out[e] = sum over parts b (in order) of partial[b * ne + e]
__global__ void __launch_bounds__(256) k_block_fold(const double *__restrict__ partial, int nparts, int ne,
                                                    double *__restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  double s = 0.0;
  for (int b = 0; b < nparts; b++) s += partial[(int64_t)b * ne + e];
  out[e] = s;
}

extern "C" int tg_block_gram(tg_vec_t x, int kx, tg_vec_t y, int ky, int64_t n, double *g_host) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(x && y && g_host, "tg_block_gram: null argument");
  TG_REQUIRE_WIDTH(kx);
  TG_REQUIRE_WIDTH(ky);
  TG_REQUIRE(n >= 0 && x->n == n * kx && y->n == n * ky, "tg_block_gram: blocks of %lld and %lld entries are not %lld x %d / %d",
             (long long)x->n, (long long)y->n, (long long)n, kx, ky);
  const int ne = kx * ky;
  if (n == 0) {
    memset(g_host, 0, sizeof(double) * ne);
    return 0;
  }
  int64_t chunk;
  int nparts;
  tg_block_parts(n, 64, &chunk, &nparts);
  double *pin = nullptr;
  TG_TRY(tg_eig_pinned(&pin));
  double *buf = nullptr;
  TG_TRY(tg_dmalloc(&buf, (int64_t)(nparts + 1) * ne));
  double *out = buf + (int64_t)nparts * ne;
  hipLaunchKernelGGL(k_block_gram, dim3(nparts), dim3(256), 0, g_tg.stream, x->d, kx, y->d, ky, n, chunk, buf);
  hipLaunchKernelGGL(k_block_fold, dim3((unsigned)tg_cdiv(ne, 256)), dim3(256), 0, g_tg.stream, buf, nparts, ne, out);
  hipError_t le = hipGetLastError();
  hipError_t ce = le == hipSuccess ? hipMemcpyAsync(pin, out, sizeof(double) * ne, hipMemcpyDeviceToHost, g_tg.stream)
                                   : le;
  hipError_t se = hipStreamSynchronize(g_tg.stream);
  tg_dfree(buf);
  TG_CHECK_HIP(ce);
  TG_CHECK_HIP(se);
  memcpy(g_host, pin, sizeof(double) * ne);
  return 0;
}

// ------------------------------------------------------------------------------------------------- combine
struct tg_comb_args {
  const double *x[3];
  const double *c[3];   // device, c[s][a * ky + j]
  int k[3];
  int nin;
};

__global__ void __launch_bounds__(256) k_block_combine(tg_comb_args args, int ky, int64_t n, double *__restrict__ Y) {
  const int64_t total = n * ky;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const int64_t i = e / ky;
    const int j = (int)(e - i * ky);
    double acc = 0.0;
    for (int s = 0; s < args.nin; s++) {
      const int ks = args.k[s];
      const double *xr = args.x[s] + i * ks;
      const double *cs = args.c[s] + j;
      for (int a = 0; a < ks; a++) acc += xr[a] * cs[a * ky];
    }
    Y[e] = acc;
  }
}

extern "C" int tg_block_combine(tg_vec_t y, int ky, int64_t n, tg_vec_t x0, int k0, const double *c0, tg_vec_t x1, int k1,
                                const double *c1, tg_vec_t x2, int k2, const double *c2) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(y, "tg_block_combine: null output");
  TG_REQUIRE_WIDTH(ky);
  TG_REQUIRE(n >= 0 && y->n == n * ky, "tg_block_combine: Y has %lld entries, not %lld x %d", (long long)y->n, (long long)n,
             ky);
  tg_vec_t xs[3] = {x0, x1, x2};
  const double *cs[3] = {c0, c1, c2};
  const int ks[3] = {k0, k1, k2};
  tg_comb_args args;
  memset(&args, 0, sizeof(args));
  int64_t ncoef = 0;
  for (int s = 0; s < 3; s++) {
    if (!xs[s]) continue;
    TG_REQUIRE(cs[s], "tg_block_combine: input %d has no coefficient matrix", s);
    TG_REQUIRE_WIDTH(ks[s]);
    TG_REQUIRE(xs[s]->n == n * ks[s], "tg_block_combine: input %d has %lld entries, not %lld x %d", s,
               (long long)xs[s]->n, (long long)n, ks[s]);
    TG_REQUIRE(xs[s]->d != y->d || n == 0, "tg_block_combine: the output must not be one of the inputs");
    args.x[args.nin] = xs[s]->d;
    args.k[args.nin] = ks[s];
    args.nin++;
    ncoef += (int64_t)ks[s] * ky;
  }
  if (n == 0) return 0;
  double *cbuf = nullptr;
  TG_TRY(tg_dmalloc(&cbuf, std::max<int64_t>(ncoef, 1)));
  std::vector<double> h((size_t)std::max<int64_t>(ncoef, 1), 0.0);
  int64_t off = 0;
  for (int s = 0, m = 0; s < 3; s++) {
    if (!xs[s]) continue;
    memcpy(h.data() + off, cs[s], sizeof(double) * ks[s] * ky);
    args.c[m++] = cbuf + off;
    off += (int64_t)ks[s] * ky;
  }
  int rc = tg_h2d_staged(cbuf, h.data(), sizeof(double) * h.size());
  if (!rc) {
    hipLaunchKernelGGL(k_block_combine, dim3(tg_grid_1d(n * ky, 256)), dim3(256), 0, g_tg.stream, args, ky, n, y->d);
    if (hipGetLastError() != hipSuccess) {
      tg_set_error("tg_block_combine: launch failed");
      rc = 1;
    }
  }
  tg_dfree(cbuf);     // (stream-ordered reuse: the allocator hands the block out again behind this launch)
  return rc;
}

// ------------------------------------------------------------------------------------------------- residual
struct tg_lam_args {
  double v[TG_BLOCK_MAX];
};

// rows [blockIdx.x * chunk, ...): thread t works on column t % k of rows t / k, t / k + per, ...; per-column sums of
// R^2 and BX^2 in a fixed order (rows in order per thread, then the threads of a column in order)
__global__ void __launch_bounds__(256)
    k_block_residual(const double *__restrict__ AX, const double *__restrict__ BX, tg_lam_args lam, int k, int64_t n,
                     int64_t chunk, const double *__restrict__ mask, const double *__restrict__ dinv, double *__restrict__ R,
                     double *__restrict__ W, double *__restrict__ partial) {
  __shared__ double lr[256], lb[256];
  const int t = threadIdx.x;
  const int per = 256 / k;
  const int rs = t / k, j = t - rs * k;
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = std::min<int64_t>(n, r0 + chunk);
  double sr = 0.0, sb = 0.0;
  if (rs < per) {
    const double l = lam.v[j];
    for (int64_t i = r0 + rs; i < r1; i += per) {
      const int64_t e = i * k + j;
      const double bx = BX[e];
      double r = AX[e] - bx * l;
      if (mask && mask[i] != 0.0) r = 0.0;
      R[e] = r;
      if (W) W[e] = dinv ? dinv[i] * r : r;
      sr += r * r;
      sb += bx * bx;
    }
  }
  lr[t] = sr;
  lb[t] = sb;
  __syncthreads();
  if (t < k) {
    double a = 0.0, b = 0.0;
    for (int q = 0; q < per; q++) {
      a += lr[q * k + t];
      b += lb[q * k + t];
    }
    partial[(int64_t)blockIdx.x * 2 * k + t] = a;
    partial[(int64_t)blockIdx.x * 2 * k + k + t] = b;
  }
}

extern "C" int tg_block_residual(tg_vec_t ax, tg_vec_t bx, const double *lam, int k, int64_t n, tg_vec_t mask, tg_vec_t dinv,
                                 tg_vec_t r, tg_vec_t w, double *rnorm2, double *bxnorm2) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(ax && bx && lam && r && rnorm2, "tg_block_residual: null argument");
  TG_REQUIRE_WIDTH(k);
  TG_REQUIRE(n >= 0 && ax->n == n * k && bx->n == n * k && r->n == n * k && (!w || w->n == n * k),
             "tg_block_residual: blocks are not %lld x %d", (long long)n, k);
  TG_REQUIRE((!mask || mask->n == n) && (!dinv || dinv->n == n), "tg_block_residual: mask / diagonal is not of length %lld",
             (long long)n);
  TG_REQUIRE(!dinv || w, "tg_block_residual: a diagonal without an output W");
  TG_REQUIRE(n == 0 || (r->d != ax->d && r->d != bx->d && (!w || (w->d != ax->d && w->d != bx->d && w->d != r->d))),
             "tg_block_residual: outputs must not alias inputs or each other");
  if (n == 0) {
    for (int j = 0; j < k; j++) {
      rnorm2[j] = 0.0;
      if (bxnorm2) bxnorm2[j] = 0.0;
    }
    return 0;
  }
  tg_lam_args la;
  memset(&la, 0, sizeof(la));
  for (int j = 0; j < k; j++) la.v[j] = lam[j];
  int64_t chunk;
  int nparts;
  tg_block_parts(n, 64, &chunk, &nparts);
  double *pin = nullptr;
  TG_TRY(tg_eig_pinned(&pin));
  double *buf = nullptr;
  TG_TRY(tg_dmalloc(&buf, (int64_t)(nparts + 1) * 2 * k));
  double *out = buf + (int64_t)nparts * 2 * k;
  hipLaunchKernelGGL(k_block_residual, dim3(nparts), dim3(256), 0, g_tg.stream, ax->d, bx->d, la, k, n, chunk,
                     mask ? mask->d : nullptr, dinv ? dinv->d : nullptr, r->d, w ? w->d : nullptr, buf);
  hipLaunchKernelGGL(k_block_fold, dim3(1), dim3(256), 0, g_tg.stream, buf, nparts, 2 * k, out);
  hipError_t le = hipGetLastError();
  hipError_t ce = le == hipSuccess ? hipMemcpyAsync(pin, out, sizeof(double) * 2 * k, hipMemcpyDeviceToHost, g_tg.stream)
                                   : le;
  hipError_t se = hipStreamSynchronize(g_tg.stream);
  tg_dfree(buf);
  TG_CHECK_HIP(ce);
  TG_CHECK_HIP(se);
  for (int j = 0; j < k; j++) {
    rnorm2[j] = pin[j];
    if (bxnorm2) bxnorm2[j] = pin[k + j];
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------- columns
__global__ void __launch_bounds__(256) k_block_column(double *__restrict__ blk, int k, int j, double *__restrict__ v,
                                                      int64_t n, int to_block) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (to_block)
      blk[i * k + j] = v[i];
    else
      v[i] = blk[i * k + j];
  }
}

static int tg_block_column(tg_vec_t x, int k, int j, tg_vec_t v, int to_block) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(x && v, "tg_block_get/set_column: null argument");
  TG_REQUIRE_WIDTH(k);
  TG_REQUIRE(j >= 0 && j < k, "tg_block_get/set_column: column %d outside [0, %d)", j, k);
  TG_REQUIRE(x->n == v->n * k, "tg_block_get/set_column: block of %lld entries, vector of %lld, width %d", (long long)x->n,
             (long long)v->n, k);
  if (v->n == 0) return 0;
  hipLaunchKernelGGL(k_block_column, dim3(tg_grid_1d(v->n, 256)), dim3(256), 0, g_tg.stream, x->d, k, j, v->d, v->n,
                     to_block);
  TG_LAUNCH_CHECK();
  return 0;
}

extern "C" int tg_block_get_column(tg_vec_t x, int k, int j, tg_vec_t v) { return tg_block_column(x, k, j, v, 0); }
extern "C" int tg_block_set_column(tg_vec_t x, int k, int j, tg_vec_t v) { return tg_block_column(x, k, j, v, 1); }

// ------------------------------------------------------------------------------------------------- decoupled rows
// one wave per row: off-diagonal non-zeros of A's row (and B's) and the diagonals
__global__ void __launch_bounds__(256)
    k_decoupled(const int64_t *__restrict__ arp, const int32_t *__restrict__ acol, const double *__restrict__ aval,
                const int64_t *__restrict__ brp, const int32_t *__restrict__ bcol, const double *__restrict__ bval,
                int64_t n, double *__restrict__ mark, double *__restrict__ da, double *__restrict__ db,
                unsigned long long *count) {   // count[0] rows marked, count[1] bits of the largest sum |a_ij| of an unmarked row
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < n; r += nwaves) {
    bool off = false;
    double dga = 0.0, dgb = 1.0, rsum = 0.0;
    for (int64_t q = arp[r] + lane; q < arp[r + 1]; q += 64) {
      rsum += fabs(aval[q]);
      if (acol[q] == r) dga += aval[q];
      else if (aval[q] != 0.0) off = true;
    }
    dga = tg_wave_sum(dga);
    rsum = tg_wave_sum(rsum);
    if (brp) {
      dgb = 0.0;
      for (int64_t q = brp[r] + lane; q < brp[r + 1]; q += 64) {
        if (bcol[q] == r) dgb += bval[q];
        else if (bval[q] != 0.0) off = true;
      }
      dgb = tg_wave_sum(dgb);
    }
    const bool any_off = __any(off);
    if (lane == 0) {                           // (tg_wave_sum: the sums are complete in lane 0)
      mark[r] = any_off ? 0.0 : 1.0;
      da[r] = dga;
      if (db) db[r] = dgb;
      if (!any_off) atomicAdd(&count[0], 1ull);
      else if (rsum > 0.0) atomicMax(&count[1], (unsigned long long)__double_as_longlong(rsum));   // (integer max: any order)
    }
  }
}

extern "C" int tg_csr_decoupled_rows(tg_csr_t a, tg_csr_t b, tg_vec_t mark, tg_vec_t da, tg_vec_t db, int64_t *count,
                                     double *arow) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(a && mark && da && count, "tg_csr_decoupled_rows: null argument");
  TG_REQUIRE(!a->rowcnt && !a->view && (!b || (!b->rowcnt && !b->view)), "tg_csr_decoupled_rows: loose-row or view CSR");
  TG_REQUIRE(a->nrows == a->ncols && (!b || (b->nrows == a->nrows && b->ncols == a->ncols)),
             "tg_csr_decoupled_rows: A and B must be square and of one size");
  const int64_t n = a->nrows;
  TG_REQUIRE(mark->n == n && da->n == n && (!db || db->n == n), "tg_csr_decoupled_rows: outputs are not of length %lld",
             (long long)n);
  *count = 0;
  if (arow) *arow = 0.0;
  if (n == 0) return 0;
  unsigned long long *cnt = nullptr;
  TG_TRY(tg_dmalloc(&cnt, 2));
  hipError_t me = hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned long long), g_tg.stream);
  if (me == hipSuccess) {
    const unsigned grid = (unsigned)std::min<int64_t>(tg_cdiv(n, 4), (int64_t)g_tg.num_cu * 8);
    hipLaunchKernelGGL(k_decoupled, dim3(grid), dim3(256), 0, g_tg.stream, a->rowptr, a->col, a->val,
                       b ? b->rowptr : nullptr, b ? b->col : nullptr, b ? b->val : nullptr, n, mark->d, da->d,
                       db ? db->d : nullptr, cnt);
    me = hipGetLastError();
  }
  if (me == hipSuccess)
    me = hipMemcpyAsync(g_tg.host_pinned, cnt, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, g_tg.stream);
  hipError_t se = hipStreamSynchronize(g_tg.stream);
  tg_dfree(cnt);
  TG_CHECK_HIP(me);
  TG_CHECK_HIP(se);
  unsigned long long c[2];
  memcpy(c, g_tg.host_pinned, sizeof(c));
  *count = (int64_t)c[0];
  if (arow) memcpy(arow, &c[1], sizeof(double));
  return 0;
}

// ------------------------------------------------------------------------------------------------- symmetry
// thread per row: merge of row r of A and row r of A^T (columns ascending in both); max |difference|, max |off-diagonal
// entry| as the bits of non-negative doubles (integer max: order-independent); unsorted[0] = 1 when a row of A is not ascending
__global__ void __launch_bounds__(256)
    k_sym_defect(const int64_t *__restrict__ arp, const int32_t *__restrict__ acol, const double *__restrict__ aval,
                 const int64_t *__restrict__ trp, const int32_t *__restrict__ tcol, const double *__restrict__ tval,
                 int64_t n, unsigned long long *out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    int64_t p = arp[r], pe = arp[r + 1], q = trp[r], qe = trp[r + 1];
    double dmax = 0.0, amax = 0.0;
    int32_t last = -1;
    bool unsorted = false;
    while (p < pe || q < qe) {
      const int32_t ca = p < pe ? acol[p] : 0x7fffffff, ct = q < qe ? tcol[q] : 0x7fffffff;
      double d;
      if (ca == ct) {
        d = aval[p] - tval[q];
        if (ca != r) amax = fmax(amax, fabs(aval[p]));
        if (ca < last) unsorted = true;
        last = ca;
        p++;
        q++;
      } else if (ca < ct) {
        d = aval[p];
        if (ca != r) amax = fmax(amax, fabs(aval[p]));
        if (ca < last) unsorted = true;
        last = ca;
        p++;
      } else {
        d = tval[q];
        q++;
      }
      dmax = fmax(dmax, fabs(d));
    }
    if (dmax > 0.0 || dmax != dmax) atomicMax(&out[0], (unsigned long long)__double_as_longlong(dmax != dmax ? INFINITY : dmax));
    if (amax > 0.0) atomicMax(&out[1], (unsigned long long)__double_as_longlong(amax));
    if (unsorted) atomicMax(&out[2], 1ull);
  }
}

extern "C" int tg_csr_sym_defect(tg_csr_t a, tg_csr_t at, double *defect, double *amax, int *unsorted) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(a && at && defect && amax && unsorted, "tg_csr_sym_defect: null argument");
  TG_REQUIRE(!a->rowcnt && !a->view && !at->rowcnt && !at->view, "tg_csr_sym_defect: loose-row or view CSR");
  TG_REQUIRE(a->nrows == a->ncols && at->nrows == a->nrows && at->ncols == a->ncols,
             "tg_csr_sym_defect: A and its transpose must be square and of one size");
  *defect = 0.0;
  *amax = 0.0;
  *unsorted = 0;
  if (a->nrows == 0) return 0;
  unsigned long long *buf = nullptr;
  TG_TRY(tg_dmalloc(&buf, 3));
  hipError_t me = hipMemsetAsync(buf, 0, 3 * sizeof(unsigned long long), g_tg.stream);
  if (me == hipSuccess) {
    hipLaunchKernelGGL(k_sym_defect, dim3(tg_grid_1d(a->nrows, 256)), dim3(256), 0, g_tg.stream, a->rowptr, a->col, a->val,
                       at->rowptr, at->col, at->val, a->nrows, buf);
    me = hipGetLastError();
  }
  if (me == hipSuccess)
    me = hipMemcpyAsync(g_tg.host_pinned, buf, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, g_tg.stream);
  hipError_t se = hipStreamSynchronize(g_tg.stream);
  tg_dfree(buf);
  TG_CHECK_HIP(me);
  TG_CHECK_HIP(se);
  unsigned long long h[3];
  memcpy(h, g_tg.host_pinned, sizeof(h));
  memcpy(defect, &h[0], sizeof(double));
  memcpy(amax, &h[1], sizeof(double));
  *unsorted = h[2] ? 1 : 0;
  return 0;
}
