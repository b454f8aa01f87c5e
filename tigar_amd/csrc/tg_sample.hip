// Evaluation at points the caller chooses, and the closest point of a patch to a physical point: the exits of a solution
// that the Gauss points of tg_postproc.hip do not give (probes, comparison on a regular grid, transfer to another mesh, the
// closest-point projection of contact).  Patches are the tg_patch_t of the point kernels (one mapped tensor-product patch,
// continuous Q_p fields on the node grid, geometry F = cp[i]/cp[nsd], d = 1, 2, 3, nsd >= d); patch->nq is not read.
//
//   tg_point_eval     x = F(xi), u_h(xi) of nF fields and their Cartesian gradients DF g^-1 grad_xi at npts parametric points
//   tg_point_locate   argmin |x - F(xi)|^2 over the parametric box by damped Gauss-Newton steps with an active set
//
// ONE LANE PER POINT.  A point's element is found by bisection in the element vertices (largest e <= nel - 1 with v[e] <=
// xi: a point on an interior vertex belongs to the upper element, the last vertex to the last element; exact comparisons),
// its local coordinate is t = (xi - v[e]) / (v[e+1] - v[e]), kept as an unevaluated sum of two doubles so that a point next
// to a Lagrange node keeps the relative accuracy of the functions that vanish there.  The 1-D tables l[k][a], l'[k][a] of the equispaced Lagrange
// basis at t are per lane: for p <= 4 the kernels are instantiated per (d, p) and the tables are registers (every index is a
// constant after unrolling); the generic route (p <= 8 wherever (p+1)^d <= TG_ASM_MAXLOC) keeps them in LDS, 64 lanes per
// workgroup, entry i of lane t at i * 64 + t.  The loops over d and p are uniform, only the addresses diverge.  Everything
// is formed in the coordinates of the reference element as in k_postproc (the Cartesian gradient is the same vector in any
// parametrisation); the projection scales DF to the knot coordinates.  Grids are capped (TG_SP_MAX_BLOCKS workgroups) and
// stride over the rest.  No atomics of any kind, no reduction across lanes: a point's result depends on that point alone,
// and the same inputs give the same bits.
//
// The seed search of the projection stages the physical centres of the seed elements through LDS in tiles of
// TG_SP_SEED_TILE and compares by brute force, ties to the lowest seed index.
//
// The patch check is tg_point_shared.h's, the inverse of the (scaled) normal matrix tg_asm_shared.h's tg_sym_inverse.
#include "tg_common.h"
#include "tg_point_shared.h"
#include <cmath>
#include <utility>

#define TG_SP_MAXP1 (TG_MAX_DEGREE + 1)
#define TG_SP_BLOCK 256            // lanes per workgroup, tables in registers (p <= 4)
#define TG_SP_BLOCK_GENERIC 64     // ... tables in LDS
#define TG_SP_MAX_BLOCKS 1024      // workgroups of a launch; the points beyond are reached by the stride loop
#define TG_SP_SEED_TILE 256        // seed centres per LDS tile
#define TG_SP_MAX_HALVINGS 10
#define TG_SP_MAX_ITER 100
#define TG_SP_SINGULAR 1e-20       // det of the scaled normal matrix relative to (its largest diagonal entry)^d
#define TG_SP_SLACK 32.0           // |r|^2 "does not decrease" beyond this many eps (|x_c| + |F_c|) per component

struct tg_sp_patch {               // what the kernels see of a patch
  int d, p, nsd;
  int nel[3], n[3];
  const double *verts[3];          // device copies of the element vertices
  const double *f[4];              // 0..2 the homogeneous coordinates (the first nsd), 3 the weight function
  const double *lag;               // generic route: 1 / prod_{m != a} (a - m), a = 0 .. p
};

// 1 / prod_{m != a} (a - m): the denominator of l_a in the variable z = p t, whose nodes are the integers 0 .. p
__host__ __device__ constexpr double tg_sp_cden(int p, int a) {
  int c = 1;
  for (int m = 0; m <= p; m++)
    if (m != a) c *= a - m;
  return 1.0 / c;
}

// per-lane 1-D tables: registers (constant indices after unrolling) or LDS (lane-strided)
template <int D, int P1>
struct tg_sp_regtab {
  double l[D][P1], dl[D][P1];
  __device__ __forceinline__ double L(int k, int a) const { return l[k][a]; }
  __device__ __forceinline__ double DL(int k, int a) const { return dl[k][a]; }
  __device__ __forceinline__ void set(int k, int a, double v, double dv) {
    l[k][a] = v;
    dl[k][a] = dv;
  }
};
struct tg_sp_ldstab {
  double *b;                       // this lane's first entry
  int nt, p1;
  __device__ __forceinline__ double L(int k, int a) const { return b[(size_t)((2 * k) * p1 + a) * nt]; }
  __device__ __forceinline__ double DL(int k, int a) const { return b[(size_t)((2 * k + 1) * p1 + a) * nt]; }
  __device__ __forceinline__ void set(int k, int a, double v, double dv) {
    b[(size_t)((2 * k) * p1 + a) * nt] = v;
    b[(size_t)((2 * k + 1) * p1 + a) * nt] = dv;
  }
};
template <int D, int PT>
struct tg_sp_tab_of {
  typedef tg_sp_regtab<D, PT + 1> type;
};
template <int D>
struct tg_sp_tab_of<D, 0> {
  typedef tg_sp_ldstab type;
};

// a - b as an unevaluated sum hi + lo (Knuth's two-sum: exact)
__device__ __forceinline__ void tg_sp_two_diff(double a, double b, double *hi, double *lo) {
#pragma clang fp contract(off)
  const double s = a - b, bb = s - a;
  *hi = s;
  *lo = (a - (s - bb)) - (b + bb);
}

// element of xi in direction k and z = p t, t = (xi - v[e]) / (v[e+1] - v[e]), as an unevaluated sum z_hi + z_lo: next to
// a node (z near an integer) the factor z - m of the Lagrange functions would otherwise carry the rounding of t at full size.
// No contraction here or in tg_sp_factor: z_hi must be the ROUNDED product p t_hi, whose rounding z_lo holds -- fused into
// fma(p, t_hi, -m) the factor would count that rounding twice (the device compiler did; seen as 58 x the bound at p = 3).
// The bisection stays inside [0, nel - 1] whatever xi is
__device__ __forceinline__ void tg_sp_element(const double *v, int nel, int p, double xi, int *e, double *z_hi, double *z_lo, double *h) {
#pragma clang fp contract(off)
  int lo = 0, hi = nel - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (v[mid] <= xi)
      lo = mid;
    else
      hi = mid - 1;
  }
  const double v0 = v[lo];
  double h_hi, h_lo, s_hi, s_lo;
  tg_sp_two_diff(v[lo + 1], v0, &h_hi, &h_lo);
  tg_sp_two_diff(xi, v0, &s_hi, &s_lo);
  const double t_hi = s_hi / h_hi;
  const double t_lo = (fma(-t_hi, h_hi, s_hi) + (s_lo - t_hi * h_lo)) / h_hi;        // (the remainder of the division is exact)
  const double pd = (double)p, z = pd * t_hi;
  *e = lo;
  *h = h_hi;
  *z_hi = z;
  *z_lo = fma(pd, t_hi, -z) + pd * t_lo;
}

__device__ __forceinline__ double tg_sp_factor(double z_hi, double z_lo, int m) {
#pragma clang fp contract(off)
  return (z_hi - (double)m) + z_lo;
}

// i = 0 .. n - 1 with constant indices where the count is known at compile time (N > 0: the tables are registers), a plain
// loop otherwise
template <class F, int... I>
__device__ __forceinline__ void tg_sp_for_seq(F &f, std::integer_sequence<int, I...>) {
  (f(I), ...);
}
template <int N, class F>
__device__ __forceinline__ void tg_sp_for(int n, F f) {
  if constexpr (N > 0)
    tg_sp_for_seq(f, std::make_integer_sequence<int, N>{});
  else
    for (int i = 0; i < n; i++) f(i);
}

// l_a = c_a prod_{m != a} (z - m), d l_a / d t = p c_a sum_{m != a} prod_{r != a, m} (z - r), z = p t: integer nodes, each factor
// (z_hi - m) + z_lo
template <int PT, class TAB>
__device__ __forceinline__ void tg_sp_fill(const tg_sp_patch &S, int k, double z_hi, double z_lo, TAB &T) {
  constexpr int P1 = PT ? PT + 1 : 0, PN = PT ? PT : 1;
  const int p1 = PT ? PT + 1 : S.p + 1;
  tg_sp_for<P1>(p1, [&](int a) {
    double l = 1.0, dl = 0.0;
    tg_sp_for<P1>(p1, [&](int m) {
      if (m == a) return;
      l *= tg_sp_factor(z_hi, z_lo, m);
      double term = 1.0;
      tg_sp_for<P1>(p1, [&](int r) {
        if (r != a && r != m) term *= tg_sp_factor(z_hi, z_lo, r);
      });
      dl += term;
    });
    const double c = PT ? tg_sp_cden(PN, a) : S.lag[a];
    T.set(k, a, l * c, dl * (c * (double)(p1 - 1)));
  });
}

// value and reference-element derivatives of one nodal field at the point: one contraction per direction
template <int D, int PT, class TAB>
__device__ __forceinline__ void tg_sp_contract(const tg_sp_patch &S, const double *f, int64_t node0, const TAB &T, double &v,
                                               double (&g)[3]) {
  constexpr int P1 = PT ? PT + 1 : 0;
  const int p1 = PT ? PT + 1 : S.p + 1;
  const int64_t s1 = S.n[0], s2 = (int64_t)S.n[0] * S.n[1];
  double v2 = 0.0, g20 = 0.0, g21 = 0.0, g22 = 0.0;
  tg_sp_for<(D > 2 ? P1 : 1)>(D > 2 ? p1 : 1, [&](int a2) {
    double v1 = 0.0, g10 = 0.0, g11 = 0.0;
    tg_sp_for<(D > 1 ? P1 : 1)>(D > 1 ? p1 : 1, [&](int a1) {
      const double *row = f + node0 + a1 * s1 + a2 * s2;
      double v0 = 0.0, g00 = 0.0;
      tg_sp_for<P1>(p1, [&](int a0) {
        const double x = row[a0];
        v0 = fma(T.L(0, a0), x, v0);
        g00 = fma(T.DL(0, a0), x, g00);
      });
      if constexpr (D > 1) {
        v1 = fma(T.L(1, a1), v0, v1);
        g10 = fma(T.L(1, a1), g00, g10);
        g11 = fma(T.DL(1, a1), v0, g11);
      } else {
        v1 = v0;
        g10 = g00;
      }
    });
    if constexpr (D > 2) {
      v2 = fma(T.L(2, a2), v1, v2);
      g20 = fma(T.L(2, a2), g10, g20);
      g21 = fma(T.L(2, a2), g11, g21);
      g22 = fma(T.DL(2, a2), v1, g22);
    } else {
      v2 = v1;
      g20 = g10;
      g21 = g11;
    }
  });
  v = v2;
  g[0] = g20;
  g[1] = g21;
  g[2] = g22;
}

// elements, tables and first local node of the point xi (inside the box); h: the element sizes
template <int D, int PT, class TAB>
__device__ __forceinline__ int64_t tg_sp_place(const tg_sp_patch &S, const double (&xi)[3], TAB &T, double (&h)[3]) {
  int64_t node0 = 0, stride = 1;
#pragma unroll
  for (int k = 0; k < D; k++) {
    int e;
    double z_hi, z_lo;
    tg_sp_element(S.verts[k], S.nel[k], S.p, xi[k], &e, &z_hi, &z_lo, &h[k]);
    tg_sp_fill<PT>(S, k, z_hi, z_lo, T);
    node0 += stride * ((int64_t)e * S.p);
    stride *= S.n[k];
  }
  return node0;
}

// x = N / W and DF[c][k] = d(N_c / W)/dt_k in the coordinates of the reference element (zero beyond nsd, d); the
// expressions of k_postproc
template <int D, int PT, class TAB>
__device__ __forceinline__ void tg_sp_geometry(const tg_sp_patch &S, int64_t node0, const TAB &T, double (&X)[3], double (&DF)[3][3],
                                               double &W, double (&dW)[3]) {
  tg_sp_contract<D, PT>(S, S.f[3], node0, T, W, dW);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    X[c] = 0.0;
    DF[c][0] = DF[c][1] = DF[c][2] = 0.0;
    if (c >= S.nsd) continue;
    double N, dN[3];
    tg_sp_contract<D, PT>(S, S.f[c], node0, T, N, dN);
    X[c] = N / W;
#pragma unroll
    for (int k = 0; k < D; k++) DF[c][k] = (dN[k] * W - N * dW[k]) / (W * W);
  }
}

struct tg_sp_eval_args {
  tg_sp_patch S;
  int nF, rational;
  const double *u;                 // nF fields of nnodes values (may be null)
  int64_t nnodes, npts;
  const double *xi;
  double *x, *val, *grad;          // any may be null
};

template <int D, int PT>
__global__ void __launch_bounds__(PT ? TG_SP_BLOCK : TG_SP_BLOCK_GENERIC) k_point_eval(tg_sp_eval_args A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const tg_sp_patch &S = A.S;
  const int nt = blockDim.x, tid = threadIdx.x, nsd = S.nsd;
  typename tg_sp_tab_of<D, PT>::type T;
  if constexpr (PT == 0) {
    T.b = reinterpret_cast<double *>(smem) + tid;
    T.nt = nt;
    T.p1 = S.p + 1;
  }
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int64_t q = (int64_t)blockIdx.x * nt + tid; q < A.npts; q += (int64_t)gridDim.x * nt) {
    double xi[3] = {0.0, 0.0, 0.0};
    bool inside = true;
#pragma unroll
    for (int k = 0; k < D; k++) {
      xi[k] = A.xi[(int64_t)k * A.npts + q];
      inside = inside && xi[k] >= S.verts[k][0] && xi[k] <= S.verts[k][S.nel[k]];     // (false for NaN)
    }
    if (!inside) {                 // NaN everywhere; no field is read
#pragma unroll
      for (int c = 0; c < 3; c++)
        if (A.x && c < nsd) A.x[(int64_t)c * A.npts + q] = nan;
      for (int i = 0; i < A.nF && A.u; i++) {
        if (A.val) A.val[(int64_t)i * A.npts + q] = nan;
#pragma unroll
        for (int c = 0; c < 3; c++)
          if (A.grad && c < nsd) A.grad[((int64_t)i * nsd + c) * A.npts + q] = nan;
      }
      continue;
    }
    double h[3] = {1.0, 1.0, 1.0};
    const int64_t node0 = tg_sp_place<D, PT>(S, xi, T, h);
    double X[3], DF[3][3], W, dW[3];
    tg_sp_geometry<D, PT>(S, node0, T, X, DF, W, dW);
#pragma unroll
    for (int c = 0; c < 3; c++)
      if (A.x && c < nsd) A.x[(int64_t)c * A.npts + q] = X[c];
    if (!A.u || (!A.val && !A.grad)) continue;
    double gi[3][3];
    if (A.grad) {
      double G[3][3];
#pragma unroll
      for (int k = 0; k < 3; k++)
#pragma unroll
        for (int m = 0; m < 3; m++) G[k][m] = DF[0][k] * DF[0][m] + DF[1][k] * DF[1][m] + DF[2][k] * DF[2][m];
      tg_point_metric_inverse<true>(D, G, gi);
    }
    for (int i = 0; i < A.nF; i++) {
      double v, dv[3];
      tg_sp_contract<D, PT>(S, A.u + (int64_t)i * A.nnodes, node0, T, v, dv);
      if (A.rational) {            // the difference first, with one rounding, then the division (k_postproc)
        const double rw = 1.0 / W;
#pragma unroll
        for (int k = 0; k < D; k++) dv[k] = fma(dv[k], W, -(v * dW[k])) * (rw * rw);
        v *= rw;
      }
      if (A.val) A.val[(int64_t)i * A.npts + q] = v;
      if (A.grad) {
        double t[3];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = gi[k][0] * dv[0] + gi[k][1] * dv[1] + gi[k][2] * dv[2];
#pragma unroll
        for (int c = 0; c < 3; c++)
          if (c < nsd) A.grad[((int64_t)i * nsd + c) * A.npts + q] = DF[c][0] * t[0] + DF[c][1] * t[1] + DF[c][2] * t[2];
      }
    }
  }
}

// ---- closest point -----------------------------------------------------------------------------------------------------
struct tg_sp_locate_args {
  tg_sp_patch S;
  const double *x, *guess;         // nsd npts physical points; d npts starting values or null
  int64_t npts;
  double tol;
  int max_iter;
  const double *seed_xi, *seed_x;  // d nseeds parametric centres and nsd nseeds physical ones (without a guess)
  int64_t nseeds;
  double *xi_out, *info;           // d npts; distance | iterations | status
};

// the centres of the seed elements: every stride[k]-th element of direction k, seeds lexicographic with direction 0 fastest
__global__ void __launch_bounds__(256) k_seed_centres(tg_sp_patch S, int s0, int s1, int s2, int c0, int c1, int64_t nseeds, double *out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nseeds; i += (int64_t)gridDim.x * blockDim.x) {
    const int j[3] = {(int)(i % c0), (int)((i / c0) % c1), (int)(i / ((int64_t)c0 * c1))};
    const int st[3] = {s0, s1, s2};
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (k >= S.d) continue;
      const int e = j[k] * st[k];
      out[(int64_t)k * nseeds + i] = 0.5 * (S.verts[k][e] + S.verts[k][e + 1]);
    }
  }
}

// F and d F / d xi (knot coordinates) at xi, which lies inside the box
template <int D, int PT, class TAB>
__device__ __forceinline__ void tg_sp_map(const tg_sp_patch &S, const double (&xi)[3], TAB &T, double (&X)[3], double (&DF)[3][3]) {
  double h[3] = {1.0, 1.0, 1.0}, W, dW[3];
  const int64_t node0 = tg_sp_place<D, PT>(S, xi, T, h);
  tg_sp_geometry<D, PT>(S, node0, T, X, DF, W, dW);
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int k = 0; k < D; k++) DF[c][k] /= h[k];
}

// |x - F|^2 with the residual, and the slack below which a change of it is rounding
__device__ __forceinline__ double tg_sp_residual(int nsd, const double (&x)[3], const double (&X)[3], double (&r)[3], double *slack) {
  double f = 0.0, s = 0.0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    r[c] = 0.0;
    if (c >= nsd) continue;
    r[c] = x[c] - X[c];
    f = fma(r[c], r[c], f);
    const double e = (TG_SP_SLACK * 2.220446049250313e-16) * (fabs(x[c]) + fabs(X[c]));
    s = fma(e, 2.0 * fabs(r[c]) + e, s);
  }
  *slack = s;
  return f;
}

template <int D, int PT>
__global__ void __launch_bounds__(PT ? TG_SP_BLOCK : TG_SP_BLOCK_GENERIC) k_point_locate(tg_sp_locate_args A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const tg_sp_patch &S = A.S;
  const int nt = blockDim.x, tid = threadIdx.x, nsd = S.nsd;
  double *tile = reinterpret_cast<double *>(smem);                      // [nsd][TG_SP_SEED_TILE] (without a guess)
  typename tg_sp_tab_of<D, PT>::type T;
  if constexpr (PT == 0) {
    T.b = tile + (A.guess ? 0 : nsd * TG_SP_SEED_TILE) + tid;
    T.nt = nt;
    T.p1 = S.p + 1;
  }
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int64_t base = (int64_t)blockIdx.x * nt; base < A.npts; base += (int64_t)gridDim.x * nt) {
    const int64_t q = base + tid;
    const bool active = q < A.npts;
    double x[3] = {0.0, 0.0, 0.0}, xi[3] = {0.0, 0.0, 0.0};
    bool finite = active;
#pragma unroll
    for (int c = 0; c < 3; c++)
      if (active && c < nsd) {
        x[c] = A.x[(int64_t)c * A.npts + q];
        finite = finite && isfinite(x[c]);
      }
    if (A.guess) {
#pragma unroll
      for (int k = 0; k < D; k++)
        if (active) {
          xi[k] = A.guess[(int64_t)k * A.npts + q];
          finite = finite && isfinite(xi[k]);
        }
    } else {
      // nearest seed centre: the tiles pass through LDS, every lane of the workgroup walks every tile (uniform barriers)
      double best = INFINITY;
      int64_t bi = 0;
      for (int64_t s0 = 0; s0 < A.nseeds; s0 += TG_SP_SEED_TILE) {
        const int cnt = A.nseeds - s0 < TG_SP_SEED_TILE ? (int)(A.nseeds - s0) : TG_SP_SEED_TILE;
        for (int i = tid; i < cnt * nsd; i += nt) {
          const int c = i / cnt, j = i - c * cnt;
          tile[c * TG_SP_SEED_TILE + j] = A.seed_x[(int64_t)c * A.nseeds + s0 + j];
        }
        __syncthreads();
        if (finite)
          for (int j = 0; j < cnt; j++) {
            double d2 = 0.0;
#pragma unroll
            for (int c = 0; c < 3; c++)
              if (c < nsd) {
                const double df = x[c] - tile[c * TG_SP_SEED_TILE + j];
                d2 = fma(df, df, d2);
              }
            if (d2 < best) {       // (strict: ties stay with the lowest seed index)
              best = d2;
              bi = s0 + j;
            }
          }
        __syncthreads();
      }
      if (finite)
#pragma unroll
        for (int k = 0; k < D; k++) xi[k] = A.seed_xi[(int64_t)k * A.nseeds + bi];
    }
    if (!active) continue;         // (after the barriers of this round)
    double *info = A.info + q;
    if (!finite) {
#pragma unroll
      for (int k = 0; k < D; k++) A.xi_out[(int64_t)k * A.npts + q] = nan;
      info[0] = nan;
      info[A.npts] = 0.0;
      info[2 * A.npts] = 2.0;
      continue;
    }
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0}, range[3] = {1.0, 1.0, 1.0};
#pragma unroll
    for (int k = 0; k < D; k++) {
      lo[k] = S.verts[k][0];
      hi[k] = S.verts[k][S.nel[k]];
      range[k] = hi[k] - lo[k];
      xi[k] = fmin(fmax(xi[k], lo[k]), hi[k]);
    }
    double X[3], DF[3][3], r[3], slack;
    tg_sp_map<D, PT>(S, xi, T, X, DF);
    double f = tg_sp_residual(nsd, x, X, r, &slack);
    int status = 1, iters = 0;
    for (int it = 1; it <= A.max_iter; it++) {
      iters = it;
      // scaled to the box: gh = range DF^T r, Gh = range DF^T DF range; a direction whose bound is active and whose gradient
      // points outward is held: its row and column become gmax times the identity's
      double gh[3] = {0.0, 0.0, 0.0}, Gh[3][3];
      bool held[3] = {true, true, true};
#pragma unroll
      for (int k = 0; k < D; k++) {
        gh[k] = (DF[0][k] * r[0] + DF[1][k] * r[1] + DF[2][k] * r[2]) * range[k];
        held[k] = (xi[k] <= lo[k] && gh[k] < 0.0) || (xi[k] >= hi[k] && gh[k] > 0.0);
      }
      double gmax = 0.0;
#pragma unroll
      for (int k = 0; k < 3; k++)
#pragma unroll
        for (int m = 0; m < 3; m++) {
          Gh[k][m] = 0.0;
          if (k < D && m < D && !held[k] && !held[m])
            Gh[k][m] = (DF[0][k] * DF[0][m] + DF[1][k] * DF[1][m] + DF[2][k] * DF[2][m]) * (range[k] * range[m]);
          if (k == m && k < D) gmax = fmax(gmax, Gh[k][k]);
        }
      double lim = TG_SP_SINGULAR;
#pragma unroll
      for (int k = 0; k < D; k++) {
        if (held[k]) {
          Gh[k][k] = gmax;
          gh[k] = 0.0;
        }
        lim *= gmax;
      }
      double dx[3] = {0.0, 0.0, 0.0};
      bool any_free = false;
#pragma unroll
      for (int k = 0; k < D; k++) any_free = any_free || !held[k];
      if (any_free) {
        double gi[3][3];
        const double det = tg_point_metric_inverse<true>(D, Gh, gi);
        if (!(det > lim) || !(gmax <= 1.7e308)) {  // (true for NaN as well)
          status = 3;
          break;
        }
#pragma unroll
        for (int k = 0; k < D; k++) dx[k] = (gi[k][0] * gh[0] + gi[k][1] * gh[1] + gi[k][2] * gh[2]) * range[k];
      }
      double xt[3] = {0.0, 0.0, 0.0}, step = 0.0;
#pragma unroll
      for (int k = 0; k < D; k++) {
        xt[k] = fmin(fmax(xi[k] + dx[k], lo[k]), hi[k]);
        step = fmax(step, fabs(xt[k] - xi[k]) / range[k]);
      }
      if (step <= A.tol) {         // the last step is taken as it is
#pragma unroll
        for (int k = 0; k < D; k++) xi[k] = xt[k];
        tg_sp_map<D, PT>(S, xi, T, X, DF);
        f = tg_sp_residual(nsd, x, X, r, &slack);
        status = 0;
        break;
      }
      // halve while |r|^2 does not decrease (beyond rounding)
      double lam = 1.0, Xt[3], DFt[3][3], rt[3], ft;
      bool taken = false;
      for (int hv = 0; hv <= TG_SP_MAX_HALVINGS; hv++) {
        tg_sp_map<D, PT>(S, xt, T, Xt, DFt);
        ft = tg_sp_residual(nsd, x, Xt, rt, &slack);
        if (ft <= f + slack) {
          taken = true;
          break;
        }
        lam *= 0.5;
#pragma unroll
        for (int k = 0; k < D; k++) xt[k] = fmin(fmax(xi[k] + lam * dx[k], lo[k]), hi[k]);
      }
      if (!taken) break;           // no decrease along the step: status 1
      f = ft;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        r[c] = rt[c];
        X[c] = Xt[c];
        xi[c] = xt[c];
#pragma unroll
        for (int k = 0; k < 3; k++) DF[c][k] = DFt[c][k];
      }
    }
#pragma unroll
    for (int k = 0; k < D; k++) A.xi_out[(int64_t)k * A.npts + q] = xi[k];
    info[0] = sqrt(f);
    info[A.npts] = (double)iters;
    info[2 * A.npts] = (double)status;
  }
}

// ---- host drivers ------------------------------------------------------------------------------------------------------
struct tg_sp_setup_t {
  tg_sp_patch S;
  tg_patch_dims D;
  tg_dbuf<double> tables;          // the element vertices of the d directions, then the denominators of the generic route
  int pt;                          // the degree the kernels are instantiated for, 0: the generic route
  int block;
  size_t tab_lds;                  // LDS of the per-lane tables (generic route)
};

static int tg_sp_setup(const char *who, const tg_patch_t *patch, tg_sp_setup_t *U) {
  TG_REQUIRE(patch, "%s: no patch", who);
  tg_patch_t pt = *patch;
  pt.nq = 1;                       // (not read here; the shared check wants a legal value)
  TG_TRY(tg_patch_check(who, &pt, 1, true, nullptr, &U->D));
  const tg_patch_dims &D = U->D;
  tg_sp_patch &S = U->S;
  memset(&S, 0, sizeof(S));
  S.d = D.d, S.p = D.p, S.nsd = D.nsd;
  const int p1 = D.p + 1;
  std::vector<double> host;
  for (int k = 0; k < 3; k++) {
    S.nel[k] = D.nel[k], S.n[k] = D.n[k];
    if (k >= D.d) continue;
    for (int i = 0; i + 1 < pt.nverts[k]; i++)
      TG_REQUIRE(pt.verts[k][i] < pt.verts[k][i + 1], "%s: the element vertices of direction %d do not increase", who, k);
    host.insert(host.end(), pt.verts[k], pt.verts[k] + pt.nverts[k]);
  }
  for (int a = 0; a < p1; a++) host.push_back(tg_sp_cden(D.p, a));
  TG_TRY(U->tables.alloc((int64_t)host.size()));
  TG_TRY(tg_h2d_staged(U->tables.get(), host.data(), host.size() * sizeof(double)));
  const double *at = U->tables.get();
  for (int k = 0; k < D.d; k++) {
    S.verts[k] = at;
    at += pt.nverts[k];
  }
  S.lag = at;
  for (int c = 0; c <= D.nsd; c++) S.f[c < D.nsd ? c : 3] = pt.cp[c]->d;
  U->pt = D.p <= 4 ? D.p : 0;
  U->block = U->pt ? TG_SP_BLOCK : TG_SP_BLOCK_GENERIC;
  U->tab_lds = U->pt ? 0 : (size_t)2 * D.d * p1 * TG_SP_BLOCK_GENERIC * sizeof(double);
  return 0;
}

static inline unsigned tg_sp_grid(int64_t n, int block) { return (unsigned)std::min<int64_t>(TG_SP_MAX_BLOCKS, tg_cdiv(n, block)); }

template <int D>
static void tg_sp_launch_eval_d(int pt, dim3 grid, dim3 block, size_t lds, const tg_sp_eval_args &A) {
  switch (pt) {
    case 1: hipLaunchKernelGGL((k_point_eval<D, 1>), grid, block, lds, g_tg.stream, A); break;
    case 2: hipLaunchKernelGGL((k_point_eval<D, 2>), grid, block, lds, g_tg.stream, A); break;
    case 3: hipLaunchKernelGGL((k_point_eval<D, 3>), grid, block, lds, g_tg.stream, A); break;
    case 4: hipLaunchKernelGGL((k_point_eval<D, 4>), grid, block, lds, g_tg.stream, A); break;
    default: hipLaunchKernelGGL((k_point_eval<D, 0>), grid, block, lds, g_tg.stream, A); break;
  }
}

static int tg_sp_launch_eval(const tg_sp_setup_t &U, const tg_sp_eval_args &A) {
  if (A.npts <= 0) return 0;
  const dim3 grid(tg_sp_grid(A.npts, U.block)), block(U.block);
  if (U.D.d == 1) tg_sp_launch_eval_d<1>(U.pt, grid, block, U.tab_lds, A);
  if (U.D.d == 2) tg_sp_launch_eval_d<2>(U.pt, grid, block, U.tab_lds, A);
  if (U.D.d == 3) tg_sp_launch_eval_d<3>(U.pt, grid, block, U.tab_lds, A);
  TG_LAUNCH_CHECK();
  return 0;
}

template <int D>
static void tg_sp_launch_locate_d(int pt, dim3 grid, dim3 block, size_t lds, const tg_sp_locate_args &A) {
  switch (pt) {
    case 1: hipLaunchKernelGGL((k_point_locate<D, 1>), grid, block, lds, g_tg.stream, A); break;
    case 2: hipLaunchKernelGGL((k_point_locate<D, 2>), grid, block, lds, g_tg.stream, A); break;
    case 3: hipLaunchKernelGGL((k_point_locate<D, 3>), grid, block, lds, g_tg.stream, A); break;
    case 4: hipLaunchKernelGGL((k_point_locate<D, 4>), grid, block, lds, g_tg.stream, A); break;
    default: hipLaunchKernelGGL((k_point_locate<D, 0>), grid, block, lds, g_tg.stream, A); break;
  }
}

extern "C" int tg_point_eval(const tg_patch_t *patch, int nF, tg_vec_t u_nodal, tg_vec_t xi, int rational, tg_vec_t x_out,
                             tg_vec_t val_out, tg_vec_t grad_out) {
  tg_sp_setup_t U;
  TG_TRY(tg_sp_setup("tg_point_eval", patch, &U));
  const tg_patch_dims &D = U.D;
  TG_REQUIRE(xi && xi->n % D.d == 0, "tg_point_eval: xi holds d = %d coordinates per point", D.d);
  const int64_t npts = xi->n / D.d;
  TG_REQUIRE(nF >= 1, "tg_point_eval: nF = %d; at least one field", nF);
  TG_REQUIRE(!u_nodal || u_nodal->n == (int64_t)nF * D.nnodes, "tg_point_eval: the nodal vector holds %lld values, expected nF = %d fields on %lld FE nodes",
             (long long)(u_nodal ? u_nodal->n : 0), nF, (long long)D.nnodes);
  TG_REQUIRE(!x_out || x_out->n == (int64_t)D.nsd * npts, "tg_point_eval: x_out of nsd * npts = %lld values", (long long)(D.nsd * npts));
  TG_REQUIRE(!val_out || (u_nodal && val_out->n == (int64_t)nF * npts), "tg_point_eval: val_out of nF * npts = %lld values, and a nodal vector",
             (long long)(nF * npts));
  TG_REQUIRE(!grad_out || (u_nodal && grad_out->n == (int64_t)nF * D.nsd * npts),
             "tg_point_eval: grad_out of nF * nsd * npts = %lld values, and a nodal vector", (long long)((int64_t)nF * D.nsd * npts));
  tg_sp_eval_args A;
  A.S = U.S;
  A.nF = nF, A.rational = rational != 0;
  A.u = u_nodal ? u_nodal->d : nullptr;
  A.nnodes = D.nnodes, A.npts = npts;
  A.xi = xi->d;
  A.x = x_out ? x_out->d : nullptr;
  A.val = val_out ? val_out->d : nullptr;
  A.grad = grad_out ? grad_out->d : nullptr;
  return tg_sp_launch_eval(U, A);
}

// the strides of the seed lattice: the smallest that give at most max_seeds seeds -- from (1, 1, 1), the direction with the
// most seeds (the lowest on a tie) takes the next stride until the product fits
static void tg_sp_seed_strides(int d, const int *nel, int64_t max_seeds, int *stride, int *count) {
  for (int k = 0; k < 3; k++) stride[k] = count[k] = 1;
  for (int k = 0; k < d; k++) count[k] = nel[k];
  while ((int64_t)count[0] * count[1] * count[2] > max_seeds) {
    int k = 0;
    for (int m = 1; m < d; m++)
      if (count[m] > count[k]) k = m;
    stride[k]++;
    count[k] = (int)tg_cdiv(nel[k], stride[k]);
  }
}

extern "C" int tg_point_locate(const tg_patch_t *patch, tg_vec_t x, tg_vec_t xi_guess, double tol, int max_iter, int64_t max_seeds,
                               tg_vec_t xi_out, tg_vec_t info_out) {
  tg_sp_setup_t U;
  TG_TRY(tg_sp_setup("tg_point_locate", patch, &U));
  const tg_patch_dims &D = U.D;
  TG_REQUIRE(x && x->n % D.nsd == 0, "tg_point_locate: x holds nsd = %d coordinates per point", D.nsd);
  const int64_t npts = x->n / D.nsd;
  TG_REQUIRE(tol > 0.0, "tg_point_locate: tol = %g; a positive tolerance", tol);
  TG_REQUIRE(max_iter >= 1 && max_iter <= TG_SP_MAX_ITER, "tg_point_locate: max_iter = %d; 1..%d iterations", max_iter, TG_SP_MAX_ITER);
  TG_REQUIRE(xi_guess || max_seeds >= 1, "tg_point_locate: max_seeds = %lld; at least one seed", (long long)max_seeds);
  TG_REQUIRE(!xi_guess || xi_guess->n == (int64_t)D.d * npts, "tg_point_locate: xi_guess of d * npts = %lld values", (long long)(D.d * npts));
  TG_REQUIRE(xi_out && xi_out->n == (int64_t)D.d * npts, "tg_point_locate: xi_out of d * npts = %lld values", (long long)(D.d * npts));
  TG_REQUIRE(info_out && info_out->n == 3 * npts, "tg_point_locate: info_out of 3 * npts = %lld values", (long long)(3 * npts));
  if (npts == 0) return 0;
  tg_sp_locate_args A;
  memset(&A, 0, sizeof(A));
  A.S = U.S;
  A.x = x->d;
  A.guess = xi_guess ? xi_guess->d : nullptr;
  A.npts = npts;
  A.tol = tol;
  A.max_iter = max_iter;
  A.xi_out = xi_out->d;
  A.info = info_out->d;
  tg_dbuf<double> seeds;
  size_t lds = U.tab_lds;
  if (!xi_guess) {
    int stride[3], count[3];
    tg_sp_seed_strides(D.d, D.nel, max_seeds, stride, count);
    const int64_t ns = (int64_t)count[0] * count[1] * count[2];
    TG_TRY(seeds.alloc((int64_t)(D.d + D.nsd) * ns));
    hipLaunchKernelGGL(k_seed_centres, dim3(tg_sp_grid(ns, 256)), dim3(256), 0, g_tg.stream, U.S, stride[0], stride[1], stride[2],
                       count[0], count[1], ns, seeds.get());
    TG_LAUNCH_CHECK();
    tg_sp_eval_args E;
    memset(&E, 0, sizeof(E));
    E.S = U.S;
    E.nF = 1;
    E.nnodes = D.nnodes, E.npts = ns;
    E.xi = seeds.get();
    E.x = seeds.get() + (int64_t)D.d * ns;
    TG_TRY(tg_sp_launch_eval(U, E));
    A.seed_xi = E.xi;
    A.seed_x = E.x;
    A.nseeds = ns;
    lds += (size_t)D.nsd * TG_SP_SEED_TILE * sizeof(double);
  }
  const dim3 grid(tg_sp_grid(npts, U.block)), block(U.block);
  if (D.d == 1) tg_sp_launch_locate_d<1>(U.pt, grid, block, lds, A);
  if (D.d == 2) tg_sp_launch_locate_d<2>(U.pt, grid, block, lds, A);
  if (D.d == 3) tg_sp_launch_locate_d<3>(U.pt, grid, block, lds, A);
  TG_LAUNCH_CHECK();
  return 0;
}
