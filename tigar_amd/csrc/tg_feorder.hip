// FE operands in the caller's dof order (tigar_amd/feorder.py): the caller's node coordinates are recognised as a
// permutation of the tensor node grid (tg_nodes_locate), and matrices / vectors handed in in that order are brought to
// grid order on the device (tg_csr_permute_sym, tg_vec_permute).  Inside the package everything stays in grid order.
#include "tg_common.h"
#include <algorithm>
#include <string>

struct tg_feorder_s {
  int64_t n = 0;
  int32_t *grid_of_fe = nullptr;   // device, n: grid index of the caller's row i
  int32_t *fe_of_grid = nullptr;   // device, n: its inverse
  double max_snap = 0.0;           // largest accepted distance between a coordinate and its node
  int identity = 0;
};

// status words of a locate / bijection check (device): [0] smallest (row << 8 | reason) of the offending rows,
// [1] bits of the largest accepted distance, [2] != 0 when some row is not at its own index
#define TG_FO_WORDS 3
#define TG_FO_NONE 0xffffffffffffffffull
#define TG_FO_UNCLAIMED 0x7f7f7f7f   // (hipMemset pattern: larger than any row index, rows < 2^31 - 2^24)
enum { TG_FO_OFFGRID = 1, TG_FO_OTHER_FIELD = 2, TG_FO_DUPLICATE = 3, TG_FO_BAD_FIELD = 4, TG_FO_RANGE = 5 };

#define TG_FO_MAX_DIM 3
#define TG_FO_MAX_FIELDS 16
struct tg_fo_grids {
  int d, nfields;
  int64_t axis_off[TG_FO_MAX_FIELDS][TG_FO_MAX_DIM];   // start of the axis in the packed table
  int32_t axis_len[TG_FO_MAX_FIELDS][TG_FO_MAX_DIM];
  double axis_tol[TG_FO_MAX_FIELDS][TG_FO_MAX_DIM];    // tol x smallest spacing of the axis
  int64_t field_off[TG_FO_MAX_FIELDS + 1];
};

// nearest node of the ascending axis a[0..n) to x: index, distance in *dist (NaN stays NaN: never accepted)
__device__ __forceinline__ int tg_fo_nearest(const double *__restrict__ a, int n, double x, double *dist) {
  int lo = 0, hi = n;             // first index with a[idx] >= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  int idx = min(lo, n - 1);
  double best = fabs(a[idx] - x);
  if (idx > 0) {
    const double dl = fabs(a[idx - 1] - x);
    if (dl < best) {
      best = dl;
      idx--;
    }
  }
  *dist = best;
  return idx;
}

// lexicographic index (direction 0 fastest) of x on the grid of field f, or -1; *snap = largest distance over the directions
__device__ __forceinline__ int64_t tg_fo_on_grid(const tg_fo_grids *__restrict__ G, const double *__restrict__ axes, int d, int f,
                                                 const double (&x)[TG_FO_MAX_DIM], double *snap) {
  int64_t lex = 0, stride = 1;
  double worst = 0.0;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < TG_FO_MAX_DIM; k++) {
    if (k < d) {
      double dist;
      const int len = G->axis_len[f][k];
      const int idx = tg_fo_nearest(axes + G->axis_off[f][k], len, x[k], &dist);
      if (!(dist <= G->axis_tol[f][k])) ok = false;
      worst = fmax(worst, dist);
      lex += stride * idx;
      stride *= len;
    }
  }
  *snap = worst;
  return ok ? lex : -1;
}

__device__ __forceinline__ void tg_fo_report(unsigned long long *status, int64_t row, int reason) {
  atomicMin(&status[0], ((unsigned long long)row << 8) | (unsigned long long)reason);
}

__global__ void __launch_bounds__(256)
    k_fo_locate(const tg_fo_grids *__restrict__ G, const double *__restrict__ axes, const double *__restrict__ x,
                const int32_t *__restrict__ field, int64_t nrows, int32_t *__restrict__ grid_of_fe,
                unsigned long long *__restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double snap_max = 0.0;
  const int d = G->d, nfields = G->nfields;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrows; i += stride) {
    const int f = field ? field[i] : 0;
    int64_t g = -1;
    if (f < 0 || f >= nfields) {
      tg_fo_report(status, i, TG_FO_BAD_FIELD);
    } else {
      double xi[TG_FO_MAX_DIM], snap;
#pragma unroll
      for (int k = 0; k < TG_FO_MAX_DIM; k++) xi[k] = k < d ? x[i * d + k] : 0.0;
      const int64_t lex = tg_fo_on_grid(G, axes, d, f, xi, &snap);
      if (lex >= 0) {
        g = G->field_off[f] + lex;
        snap_max = fmax(snap_max, snap);
      } else {
        int reason = TG_FO_OFFGRID;
        for (int q = 0; q < nfields; q++) {
          double s2;
          if (q != f && tg_fo_on_grid(G, axes, d, q, xi, &s2) >= 0) reason = TG_FO_OTHER_FIELD;
        }
        tg_fo_report(status, i, reason);
      }
    }
    grid_of_fe[i] = (int32_t)g;
  }
  // distances are >= 0: their bit patterns order like the numbers
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) snap_max = fmax(snap_max, __shfl_down(snap_max, o, 64));
  if ((threadIdx.x & 63) == 0 && snap_max > 0.0) atomicMax(&status[1], (unsigned long long)__double_as_longlong(snap_max));
}

// the smallest row that names a grid index claims it ...
__global__ void __launch_bounds__(256)
    k_fo_claim(const int32_t *__restrict__ grid_of_fe, int64_t n, int32_t *__restrict__ fe_of_grid,
               unsigned long long *__restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int32_t g = grid_of_fe[i];
    if (g >= 0 && g < n)
      atomicMin(&fe_of_grid[g], (int32_t)i);
    else if (g != -1)                 // (-1: already reported by the locate pass)
      tg_fo_report(status, i, TG_FO_RANGE);
  }
}
// ... and every other row that names it is a duplicate
__global__ void __launch_bounds__(256)
    k_fo_verify(const int32_t *__restrict__ grid_of_fe, int64_t n, const int32_t *__restrict__ fe_of_grid,
                unsigned long long *__restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  bool moved = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int32_t g = grid_of_fe[i];
    if (g < 0 || g >= n) continue;
    if (fe_of_grid[g] != (int32_t)i) tg_fo_report(status, i, TG_FO_DUPLICATE);
    moved |= (g != (int32_t)i);
  }
  if (__any(moved) && (threadIdx.x & 63) == 0) atomicOr(&status[2], 1ull);
}

static void tg_fo_free(tg_feorder_s *h) {
  if (!h) return;
  tg_dfree(h->grid_of_fe);
  tg_dfree(h->fe_of_grid);
  delete h;
}

// bijection check of h->grid_of_fe (device, filled) and the inverse; host_status receives the status words
static int tg_fo_invert(tg_feorder_s *h, unsigned long long *status, unsigned long long *host_status) {
  const int64_t n = h->n;
  TG_CHECK_HIP(hipMemsetAsync(h->fe_of_grid, 0x7f, (size_t)std::max<int64_t>(n, 1) * sizeof(int32_t), g_tg.stream));
  if (n > 0) {
    hipLaunchKernelGGL(k_fo_claim, dim3(tg_grid_1d(n, 256)), dim3(256), 0, g_tg.stream, h->grid_of_fe, n, h->fe_of_grid,
                       status);
    hipLaunchKernelGGL(k_fo_verify, dim3(tg_grid_1d(n, 256)), dim3(256), 0, g_tg.stream, h->grid_of_fe, n, h->fe_of_grid,
                       status);
    TG_LAUNCH_CHECK();
  }
  TG_CHECK_HIP(hipMemcpyAsync(host_status, status, TG_FO_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                              g_tg.stream));
  TG_CHECK_HIP(hipStreamSynchronize(g_tg.stream));
  return 0;
}

static int tg_fo_peek(const int32_t *dev, int64_t i, int32_t *out) {
  TG_CHECK_HIP(hipMemcpyAsync(out, dev + i, sizeof(int32_t), hipMemcpyDeviceToHost, g_tg.stream));
  TG_CHECK_HIP(hipStreamSynchronize(g_tg.stream));
  return 0;
}

extern "C" int tg_nodes_locate(int d, int nfields, const int64_t *axis_len, const double *const *axes, const double *x,
                               const int32_t *field, int64_t nrows, double tol, tg_feorder_t *out) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(out && axis_len && axes && (x || nrows == 0), "null argument to tg_nodes_locate");
  TG_REQUIRE(d >= 1 && d <= TG_FO_MAX_DIM, "tg_nodes_locate: 1 to 3 directions (got %d)", d);
  TG_REQUIRE(nfields >= 1 && nfields <= TG_FO_MAX_FIELDS, "tg_nodes_locate: 1 to %d fields (got %d)", TG_FO_MAX_FIELDS, nfields);
  TG_REQUIRE(field || nfields == 1, "tg_nodes_locate: the field of every row is needed when there are several fields");
  TG_REQUIRE(tol >= 0.0 && tol < 0.5, "tg_nodes_locate: the tolerance is a fraction of the node spacing below 0.5 (got %g)", tol);
  TG_REQUIRE(nrows >= 0, "tg_nodes_locate: negative row count");
  tg_fo_grids G;
  memset(&G, 0, sizeof(G));
  G.d = d;
  G.nfields = nfields;
  std::vector<double> packed;
  int64_t total = 0;
  for (int f = 0; f < nfields; f++) {
    G.field_off[f] = total;
    int64_t nodes = 1;
    for (int k = 0; k < d; k++) {
      const int64_t len = axis_len[f * d + k];
      const double *a = axes[f * d + k];
      TG_REQUIRE(len >= 1 && len < (1ll << 31) && a, "tg_nodes_locate: empty axis %d of field %d", k, f);
      double h = 0.0;
      for (int64_t q = 1; q < len; q++) {
        TG_REQUIRE(a[q] > a[q - 1], "tg_nodes_locate: axis %d of field %d is not strictly ascending at node %lld "
                   "(a discontinuous space has no one-to-one node grid)", k, f, (long long)q);
        h = (q == 1) ? a[q] - a[q - 1] : std::min(h, a[q] - a[q - 1]);
      }
      G.axis_off[f][k] = (int64_t)packed.size();
      G.axis_len[f][k] = (int32_t)len;
      G.axis_tol[f][k] = tol * (len > 1 ? h : 1.0);
      packed.insert(packed.end(), a, a + len);
      nodes *= len;
      TG_REQUIRE(nodes < (1ll << 31), "tg_nodes_locate: more than 2^31 nodes");
    }
    total += nodes;
  }
  G.field_off[nfields] = total;
  TG_REQUIRE(total < (1ll << 31) - (1ll << 24), "tg_nodes_locate: %lld rows; fewer than 2^31 are supported", (long long)total);
  if (nrows != total) {
    tg_set_error("tg_nodes_locate declined: wrong row count: %lld rows of coordinates for a node grid of %lld nodes",
                 (long long)nrows, (long long)total);
    return 100;
  }
  tg_feorder_s *h = new tg_feorder_s();
  h->n = nrows;
  double *d_axes = nullptr, *d_x = nullptr;
  int32_t *d_field = nullptr;
  tg_fo_grids *d_grids = nullptr;
  unsigned long long *status = nullptr, hs[TG_FO_WORDS] = {TG_FO_NONE, 0ull, 0ull};
  int rc = tg_dmalloc(&h->grid_of_fe, nrows) || tg_dmalloc(&h->fe_of_grid, nrows) || tg_dmalloc(&d_axes, (int64_t)packed.size()) ||
           tg_dmalloc(&d_x, nrows * d) || tg_dmalloc(&status, TG_FO_WORDS) || tg_dmalloc(&d_grids, 1) ||
           (field && tg_dmalloc(&d_field, nrows));
  auto copy = [&](void *dst, const void *src, size_t bytes) {
    return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g_tg.stream) == hipSuccess;
  };
  if (!rc && !(copy(d_axes, packed.data(), packed.size() * sizeof(double)) && copy(d_x, x, (size_t)nrows * d * sizeof(double)) &&
               copy(status, hs, sizeof(hs)) && copy(d_grids, &G, sizeof(G)) && (!field || copy(d_field, field, (size_t)nrows * sizeof(int32_t)))))
    rc = 1;
  if (!rc && nrows > 0) {
    hipLaunchKernelGGL(k_fo_locate, dim3(tg_grid_1d(nrows, 256)), dim3(256), 0, g_tg.stream, d_grids, d_axes, d_x, d_field, nrows,
                       h->grid_of_fe, status);
    if (hipGetLastError() != hipSuccess) rc = 1;
  }
  if (!rc) rc = tg_fo_invert(h, status, hs);
  std::string why;
  if (!rc && hs[0] != TG_FO_NONE) {
    const int64_t row = (int64_t)(hs[0] >> 8);
    const int reason = (int)(hs[0] & 0xff);
    char buf[512];
    if (reason == TG_FO_OFFGRID) {
      char pt[128];
      int at = 0;
      for (int k = 0; k < d; k++) at += snprintf(pt + at, sizeof(pt) - (size_t)at, "%s%.17g", k ? ", " : "", x[row * d + k]);
      snprintf(buf, sizeof(buf), "row %lld is off the grid: (%s) lies further than %g x the node spacing from every node of "
               "field %d", (long long)row, pt, tol, field ? (int)field[row] : 0);
    } else if (reason == TG_FO_OTHER_FIELD) {
      snprintf(buf, sizeof(buf), "row %lld is a node of another field: it is labelled field %d, whose grid has no node there",
               (long long)row, (int)field[row]);
    } else if (reason == TG_FO_BAD_FIELD) {
      snprintf(buf, sizeof(buf), "row %lld is labelled field %d; the space has fields 0..%d", (long long)row, (int)field[row],
               nfields - 1);
    } else {
      int32_t g = 0, first = 0;
      rc = tg_fo_peek(h->grid_of_fe, row, &g) || tg_fo_peek(h->fe_of_grid, g, &first);
      // same node of a field whose grid has the same shape still unclaimed: the label, not the coordinate, is wrong
      int f = 0, other = -1;
      while (f + 1 < nfields && g >= G.field_off[f + 1]) f++;
      const int64_t lex = g - G.field_off[f];
      for (int q = 0; q < nfields && !rc && other < 0; q++) {
        bool same = q != f;
        for (int k = 0; k < d && same; k++)
          same = G.axis_len[q][k] == G.axis_len[f][k] &&
                 !memcmp(axes[q * d + k], axes[f * d + k], (size_t)G.axis_len[f][k] * sizeof(double));
        int32_t holder = 0;
        if (same && !tg_fo_peek(h->fe_of_grid, G.field_off[q] + lex, &holder) && holder == TG_FO_UNCLAIMED) other = q;
      }
      if (other >= 0)
        snprintf(buf, sizeof(buf), "row %lld is a node of another field: rows %lld and %lld both name node %lld of field %d "
                 "while the same node of field %d has no row", (long long)row, (long long)first, (long long)row, (long long)lex,
                 f, other);
      else
        snprintf(buf, sizeof(buf), "two rows on one node: rows %lld and %lld both lie on node %lld of field %d", (long long)first,
                 (long long)row, (long long)lex, f);
    }
    why = buf;
  }
  hipStreamSynchronize(g_tg.stream);      // (x, field and the packed axes are host arrays)
  tg_dfree(d_axes);
  tg_dfree(d_x);
  tg_dfree(d_field);
  tg_dfree(d_grids);
  tg_dfree(status);
  if (rc) {
    tg_fo_free(h);
    tg_set_error("tg_nodes_locate failed");
    return 1;
  }
  if (!why.empty()) {
    tg_fo_free(h);
    tg_set_error("tg_nodes_locate declined: %s", why.c_str());
    return 100;
  }
  h->max_snap = __builtin_bit_cast(double, hs[1]);
  h->identity = hs[2] == 0;
  *out = h;
  return 0;
}

extern "C" int tg_feorder_from_perm(const int32_t *grid_of_fe, int64_t n, tg_feorder_t *out) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(out && n >= 0 && (grid_of_fe || n == 0), "bad arguments to tg_feorder_from_perm");
  TG_REQUIRE(n < (1ll << 31) - (1ll << 24), "tg_feorder_from_perm: %lld rows; fewer than 2^31 are supported", (long long)n);
  tg_feorder_s *h = new tg_feorder_s();
  h->n = n;
  unsigned long long *status = nullptr, hs[TG_FO_WORDS] = {TG_FO_NONE, 0ull, 0ull};
  int rc = tg_dmalloc(&h->grid_of_fe, n) || tg_dmalloc(&h->fe_of_grid, n) || tg_dmalloc(&status, TG_FO_WORDS);
  if (!rc && hipMemcpyAsync(status, hs, sizeof(hs), hipMemcpyHostToDevice, g_tg.stream) != hipSuccess) rc = 1;
  if (!rc && n > 0 &&
      hipMemcpyAsync(h->grid_of_fe, grid_of_fe, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, g_tg.stream) != hipSuccess)
    rc = 1;
  if (!rc) rc = tg_fo_invert(h, status, hs);
  hipStreamSynchronize(g_tg.stream);
  tg_dfree(status);
  if (rc || hs[0] != TG_FO_NONE) {
    tg_fo_free(h);
    if (rc) {
      tg_set_error("tg_feorder_from_perm failed");
      return 1;
    }
    tg_set_error("tg_feorder_from_perm declined: not a permutation of 0..%lld (entry %lld: %s)", (long long)n - 1,
                 (long long)(hs[0] >> 8), (hs[0] & 0xff) == TG_FO_DUPLICATE ? "its value appears twice" : "out of range");
    return 100;
  }
  h->identity = hs[2] == 0;
  *out = h;
  return 0;
}

extern "C" int tg_feorder_info(tg_feorder_t h, int64_t *n, int *identity, double *max_snap) {
  TG_REQUIRE(h, "null handle");
  if (n) *n = h->n;
  if (identity) *identity = h->identity;
  if (max_snap) *max_snap = h->max_snap;
  return 0;
}

extern "C" int tg_feorder_download(tg_feorder_t h, int32_t *grid_of_fe, int32_t *fe_of_grid) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(h, "null handle");
  if (grid_of_fe && h->n)
    TG_CHECK_HIP(hipMemcpyAsync(grid_of_fe, h->grid_of_fe, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost, g_tg.stream));
  if (fe_of_grid && h->n)
    TG_CHECK_HIP(hipMemcpyAsync(fe_of_grid, h->fe_of_grid, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost, g_tg.stream));
  TG_CHECK_HIP(hipStreamSynchronize(g_tg.stream));
  return 0;
}

extern "C" int tg_feorder_destroy(tg_feorder_t h) {
  if (!h) return 0;
  if (g_tg.ready && !g_tg.multi) hipStreamSynchronize(g_tg.stream);
  tg_fo_free(h);
  return 0;
}

// ----------------------------------------------------------------------------------------------------------------------
// y[g(i)] = x[i] (to grid) / y[i] = x[g(i)] (to caller): both as gathers through the map of the destination
__global__ void __launch_bounds__(256)
    k_fo_vec_gather(const double *__restrict__ x, const int32_t *__restrict__ src_of_dst, int64_t n, double *__restrict__ y) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = x[src_of_dst[i]];
}

extern "C" int tg_vec_permute(tg_feorder_t h, tg_vec_t x, tg_vec_t y, int to_caller) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(h && x && y, "null argument to tg_vec_permute");
  TG_REQUIRE(x->n == h->n && y->n == h->n, "tg_vec_permute: vectors of %lld and %lld entries for an order of %lld rows",
             (long long)x->n, (long long)y->n, (long long)h->n);
  TG_REQUIRE(x->d != y->d, "tg_vec_permute: in place is not supported");
  if (h->n == 0) return 0;
  hipLaunchKernelGGL(k_fo_vec_gather, dim3(tg_grid_1d(h->n, 256)), dim3(256), 0, g_tg.stream, x->d,
                     to_caller ? h->grid_of_fe : h->fe_of_grid, h->n, y->d);
  TG_LAUNCH_CHECK();
  return 0;
}

// ----------------------------------------------------------------------------------------------------------------------
// B = P A P^T, B[g(i), g(j)] = A[i, j].  Destination row r is source row s = row_src[r]; its columns are renamed through
// col_map and the row is sorted by new column on chip.  Values are copied, never added.
//
// Tier E (rows of (E/2)*64 < len <= E*64 entries, E = 1: 1..64): one wave per row.  Lane l holds the E elements
// s*64 + l as 64-bit words (new column << 32 | position in the source row): unique, so the order is total and a
// bitonic network over (register, lane) sorts them -- partner distances >= 64 are exchanges between registers of one
// lane, smaller ones lane exchanges.  The values wait in LDS (written as read: coalesced) and leave it by sorted position.
#define TG_FO_TIERS 6              // E = 1, 2, 4, 8, 16, 32: rows up to 2048 entries
#define TG_FO_MAX_ONCHIP 2048

__device__ __forceinline__ int tg_fo_tier_of(int64_t len) {   // -1: empty, TG_FO_TIERS: beyond the wave tiers
  if (len <= 0) return -1;
  if (len > TG_FO_MAX_ONCHIP) return TG_FO_TIERS;
  int t = 0;
  while ((64 << t) < len) t++;
  return t;
}

__global__ void __launch_bounds__(256)
    k_fo_row_len(const int64_t *__restrict__ arp, const int32_t *__restrict__ row_src, int64_t n, int64_t *__restrict__ len,
                 unsigned long long *__restrict__ tier_rows) {
  __shared__ unsigned int cnt[TG_FO_TIERS + 1];
  if (threadIdx.x <= TG_FO_TIERS) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    const int64_t s = row_src[r];
    const int64_t l = arp[s + 1] - arp[s];
    len[r] = l;
    const int t = tg_fo_tier_of(l);
    if (t >= 0) atomicAdd(&cnt[t], 1u);
  }
  __syncthreads();
  if (threadIdx.x <= TG_FO_TIERS && cnt[threadIdx.x]) atomicAdd(&tier_rows[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

template <int E>
__global__ void __launch_bounds__(256)
    k_fo_permute_rows(const int64_t *__restrict__ arp, const int32_t *__restrict__ ac, const double *__restrict__ av,
                      const int32_t *__restrict__ row_src, const int32_t *__restrict__ col_map, int64_t n,
                      const int64_t *__restrict__ orp, int32_t *__restrict__ oc, double *__restrict__ ov) {
  constexpr int LOGE = E == 1 ? 0 : E == 2 ? 1 : E == 4 ? 2 : E == 8 ? 3 : E == 16 ? 4 : 5;
  constexpr int LOGN = 6 + LOGE;
  __shared__ double sval[4][E * 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t nblk = (n + 3) / 4;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r = blk * 4 + w;
    int64_t a = 0, o = 0;
    int len = 0;
    if (r < n) {
      const int64_t s = row_src[r];
      a = arp[s];
      const int64_t l = arp[s + 1] - a;
      o = orp[r];
      if (l <= E * 64 && (E == 1 ? l > 0 : l > E * 32)) len = (int)l;      // this tier's rows only (wave-uniform)
    }
    unsigned long long key[E];
#pragma unroll
    for (int s = 0; s < E; s++) {
      const int q = s * 64 + lane;
      key[s] = TG_FO_NONE;
      if (q < len) {
        key[s] = ((unsigned long long)(unsigned int)col_map[ac[a + q]] << 32) | (unsigned int)q;
        sval[w][q] = av[a + q];
      }
    }
    if (len > 1) {
#pragma unroll
      for (int lk = 1; lk <= LOGN; lk++) {
#pragma unroll
        for (int lj = lk - 1; lj >= 0; lj--) {
          if (lj >= 6) {                    // partner in another register of this lane
#pragma unroll
            for (int s = 0; s < E; s++) {
              const int js = 1 << (lj - 6);
              if ((s & js) == 0) {
                const bool up = (((s * 64) >> lk) & 1) == 0;
                const unsigned long long x = key[s], y = key[s | js];
                const bool sw = (x > y) == up;
                key[s] = sw ? y : x;
                key[s | js] = sw ? x : y;
              }
            }
          } else {                          // partner in another lane
#pragma unroll
            for (int s = 0; s < E; s++) {
              const unsigned long long mine = key[s];
              const unsigned long long other = __shfl_xor(mine, 1 << lj, 64);
              const bool up = ((((s * 64) | lane) >> lk) & 1) == 0;
              const bool lower = ((lane >> lj) & 1) == 0;
              const bool keep_min = lower == up;
              key[s] = ((mine < other) == keep_min) ? mine : other;
            }
          }
        }
      }
    }
    __syncthreads();                        // the values of the row are in LDS
#pragma unroll
    for (int s = 0; s < E; s++) {
      const int q = s * 64 + lane;
      if (q < len) {
        oc[o + q] = (int32_t)(key[s] >> 32);
        ov[o + q] = sval[w][(unsigned int)key[s]];
      }
    }
    __syncthreads();                        // before the next row overwrites them
  }
}

// rows beyond the wave tiers, any length: one workgroup per row; every element counts the elements that sort before it
// (the renamed columns pass through LDS in chunks) and is written at that rank
#define TG_FO_CHUNK 2048
__global__ void __launch_bounds__(256)
    k_fo_permute_long_rows(const int64_t *__restrict__ arp, const int32_t *__restrict__ ac, const double *__restrict__ av,
                           const int32_t *__restrict__ row_src, const int32_t *__restrict__ col_map, int64_t n,
                           const int64_t *__restrict__ orp, int32_t *__restrict__ oc, double *__restrict__ ov) {
  __shared__ int32_t skey[TG_FO_CHUNK];
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t s = row_src[r];
    const int64_t a = arp[s], len = arp[s + 1] - a, o = orp[r];
    if (len <= TG_FO_MAX_ONCHIP) continue;            // (uniform per workgroup)
    for (int64_t q0 = 0; q0 < len; q0 += 256) {
      const int64_t q = q0 + threadIdx.x;
      const int32_t mine = q < len ? col_map[ac[a + q]] : 0;
      int64_t rank = 0;
      for (int64_t c0 = 0; c0 < len; c0 += TG_FO_CHUNK) {
        const int m = len - c0 < TG_FO_CHUNK ? (int)(len - c0) : TG_FO_CHUNK;
        __syncthreads();
        for (int j = threadIdx.x; j < m; j += 256) skey[j] = col_map[ac[a + c0 + j]];
        __syncthreads();
        if (q < len)
          for (int j = 0; j < m; j++) rank += (skey[j] < mine) || (skey[j] == mine && c0 + j < q);
      }
      if (q < len) {
        oc[o + rank] = mine;
        ov[o + rank] = av[a + q];
      }
    }
  }
}

template <int E>
static void tg_fo_launch_tier(tg_csr_s *a, const int32_t *row_src, const int32_t *col_map, tg_csr_s *b) {
  const unsigned grid = (unsigned)std::min<int64_t>(tg_cdiv(a->nrows, 4), (int64_t)g_tg.num_cu * 32);
  hipLaunchKernelGGL((k_fo_permute_rows<E>), dim3(grid), dim3(256), 0, g_tg.stream, a->rowptr, a->col, a->val, row_src, col_map,
                     a->nrows, b->rowptr, b->col, b->val);
}

extern "C" int tg_csr_permute_sym(tg_feorder_t h, tg_csr_t a, int inverse, tg_csr_t *out) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(h && a && out, "null argument to tg_csr_permute_sym");
  TG_REQUIRE_CANONICAL(a);
  TG_REQUIRE(a->nrows == a->ncols, "tg_csr_permute_sym: a square matrix is expected (got %lld x %lld)", (long long)a->nrows,
             (long long)a->ncols);
  TG_REQUIRE(a->nrows == h->n, "tg_csr_permute_sym: a matrix of %lld rows for an order of %lld rows", (long long)a->nrows,
             (long long)h->n);
  // forward: row r of B is row fe_of_grid[r] of A, column c becomes grid_of_fe[c]; inverse: the two maps change places
  const int32_t *row_src = inverse ? h->grid_of_fe : h->fe_of_grid;
  const int32_t *col_map = inverse ? h->fe_of_grid : h->grid_of_fe;
  const int64_t n = a->nrows;
  int64_t *len = nullptr;
  unsigned long long *tier_rows = nullptr, ht[TG_FO_TIERS + 1] = {0};
  tg_csr_s *b = nullptr;
  int64_t total = 0;
  int rc = tg_dmalloc(&len, n + 1) || tg_dmalloc(&tier_rows, TG_FO_TIERS + 1);
  if (!rc && hipMemsetAsync(tier_rows, 0, sizeof(ht), g_tg.stream) != hipSuccess) rc = 1;
  if (!rc && n > 0) {
    hipLaunchKernelGGL(k_fo_row_len, dim3(tg_grid_1d(n, 256)), dim3(256), 0, g_tg.stream, a->rowptr, row_src, n, len, tier_rows);
    if (hipGetLastError() != hipSuccess) rc = 1;
  }
  if (!rc && hipMemcpyAsync(ht, tier_rows, sizeof(ht), hipMemcpyDeviceToHost, g_tg.stream) != hipSuccess) rc = 1;
  if (!rc) rc = tg_exclusive_scan_i64(len, n, &total);          // (waits for the stream: ht is valid afterwards)
  if (!rc && total != a->nnz) {
    tg_set_error("tg_csr_permute_sym: the rows gathered hold %lld entries, the matrix %lld", (long long)total, (long long)a->nnz);
    rc = 2;
  }
  if (!rc) rc = tg_csr_alloc(n, n, total, &b);
  if (!rc && hipMemcpyAsync(b->rowptr, len, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, g_tg.stream) != hipSuccess)
    rc = 1;
  if (!rc && total > 0) {
    if (ht[0]) tg_fo_launch_tier<1>(a, row_src, col_map, b);
    if (ht[1]) tg_fo_launch_tier<2>(a, row_src, col_map, b);
    if (ht[2]) tg_fo_launch_tier<4>(a, row_src, col_map, b);
    if (ht[3]) tg_fo_launch_tier<8>(a, row_src, col_map, b);
    if (ht[4]) tg_fo_launch_tier<16>(a, row_src, col_map, b);
    if (ht[5]) tg_fo_launch_tier<32>(a, row_src, col_map, b);
    if (ht[TG_FO_TIERS]) {
      const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)g_tg.num_cu * 8);
      hipLaunchKernelGGL(k_fo_permute_long_rows, dim3(grid), dim3(256), 0, g_tg.stream, a->rowptr, a->col, a->val, row_src,
                         col_map, n, b->rowptr, b->col, b->val);
    }
    if (hipGetLastError() != hipSuccess) rc = 1;
  }
  if (hipStreamSynchronize(g_tg.stream) != hipSuccess) rc = rc ? rc : 1;
  tg_dfree(len);
  tg_dfree(tier_rows);
  if (rc) {
    if (b) tg_csr_destroy(b);
    if (rc != 2) tg_set_error("tg_csr_permute_sym failed (%lld rows, %lld entries)", (long long)n, (long long)a->nnz);
    return rc == 2 ? 2 : 1;
  }
  *out = b;
  return 0;
}
