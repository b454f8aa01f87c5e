// Fast diagonalization (FD) preconditioner for CG on tensor-product patches (Lynch-Rice-Thomas; Sangalli & Tani 2016 for
// IGA).  Per field block of K, on its free box of n_0 x ... x n_{d-1} dofs:
//
//   P     = sum_k c_k (M_{d-1} x .. x K_k x .. x M_0) + c_m (M_{d-1} x .. x M_0)      (1-D parametric IGA matrices)
//   P^-1  = (Q x .. x Q) diag(1 / (sum_k c_k lam_k[i_k] + c_m)) (Q^T x .. x Q^T),    Q_k^T M_k Q_k = I, Q_k^T K_k Q_k = lam_k
//   z     = S P^-1 S r on the box (S = D^-1/2, D = diag K / diag P, or S = I),  z_i = r_i / K_ii off the box.
//
// One application is 2d mode products, all the same kernel k_fd_mode: Y[i][c] = sum_l A[l][i] X[c][l] with l the index of
// the direction being contracted (contiguous in X) and c every other index.  The output puts c contiguous, so the layout
// rotates by one direction per pass and is back in the natural order (direction 0 fastest) after d passes.  A = Q for the
// first d passes and Q^T for the last d; Q is held padded to a multiple of 16 with exact zeros, the boxes padded the same
// way (pad entries stay exactly 0 through the passes).  Fused ends: pass 0 gathers S r out of the full residual, pass d-1
// divides by the eigenvalue sums (pseudo-inverse where the sum vanishes), pass 2d-1 scales by S and scatters into z.
// Products on v_mfma_f64_16x16x4_f64, tiles of 64 (i) x 64 (c) per workgroup of 4 waves (32 x 32 each), the contraction in
// chunks of 32 through LDS with the next chunk requested into registers before the MFMAs of the current one.  No atomics:
// every output element is one MFMA chain in a fixed order, so applications are bit-reproducible.
//
// tg_krylov_solve_fd: the PCG loop of tg_krylov.hip (tg_pcg_host) with the FD application as B; the products of K as the other
// CG solves choose them (half-storage copy of tg_symgrid.hip when it applies, else the sliced copy or CSR).
#include "tg_common.h"
#include <math.h>
#include <vector>
#include <algorithm>

typedef double fd_v4d __attribute__((ext_vector_type(4)));

#define FD_MT 64           // output rows (i) per workgroup
#define FD_NT 64           // output columns (c) per workgroup
#define FD_KB 32           // contraction chunk
#define FD_FIT_BLOCKS 512

struct fd_block {
  int d = 0;
  int64_t off = 0;                       // first dof of the field
  int64_t N[3] = {1, 1, 1};              // control grid shape (direction 0 fastest)
  int64_t lo[3] = {0, 0, 0};             // free box [lo, lo + nf)
  int nf[3] = {1, 1, 1}, np[3] = {1, 1, 1};   // free sizes, padded sizes (multiples of 16)
  double *mem = nullptr;                 // one allocation for everything below
  double *Qf[3] = {}, *Qb[3] = {};       // np x np: Qf[l][i] = Q[l][i], Qb[l][i] = Q[i][l]
  double *lam[3] = {};                   // np
  double *dk[3] = {}, *dm[3] = {};       // nf: diagonals of the 1-D stiffness / mass on the free box
  double coef[4] = {0, 0, 0, 0};         // c_0 .. c_{d-1}, c_m at [3]
  double floor = 0.0;                    // eigenvalue sums <= floor are treated as 0 (pseudo-inverse)
  double lam_max[3] = {0, 0, 0};
  int64_t box() const { return (int64_t)np[0] * np[1] * np[2]; }
};

struct tg_fd_s {
  int64_t n = 0;
  std::vector<fd_block> blocks;
  double *diag = nullptr;                // diag K (tg_fd_fit)
  double *sv = nullptr;                  // S on the free boxes, 1 / K_ii off them (tg_fd_set_coefficients)
  double *w0 = nullptr, *w1 = nullptr;   // ping-pong workspaces of the largest padded box
  int64_t wsize = 0;
  bool fitted = false, ready = false;
};

struct fd_pass {
  const double *X;
  double *Y;
  const double *A;                       // np x np, A[l][i]
  int np;                                // padded size of the contracted direction
  int64_t C;                             // product of the other padded sizes
  // fused ends
  const double *r, *sv;                  // (offset to the block's first dof)
  double *z;
  int d;
  int npd[3], nf[3];
  int64_t lo[3], N[3];
  const double *lam[3];
  double coef[4], floor;
};

// MODE 0: plain; 1: X gathered from S r (direction 0); 2: epilogue divides by the eigenvalue sums (direction d-1);
// 3: epilogue scales by S and scatters into z (direction d-1)
template <int MODE>
__global__ void __launch_bounds__(256) k_fd_mode(fd_pass P) {
  __shared__ double As[FD_KB][FD_MT];
  __shared__ double Xs[FD_NT][FD_KB + 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int nit = (P.np + FD_MT - 1) / FD_MT;
  const int64_t bid = blockIdx.x;
  const int i0 = (int)(bid % nit) * FD_MT;
  const int64_t c0 = (bid / nit) * FD_NT;
  const int wi = (wave & 1) * 32, wc = (wave >> 1) * 32;
  double ra[8], rx[8];
  auto load = [&](int l0) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int e = tid + 256 * j;
      const int ka = e >> 6, ii = e & 63;
      ra[j] = (l0 + ka < P.np && i0 + ii < P.np) ? P.A[(int64_t)(l0 + ka) * P.np + i0 + ii] : 0.0;
      const int cc = e >> 5, kx = e & 31;
      const int64_t c = c0 + cc;
      const int l = l0 + kx;
      double v = 0.0;
      if (c < P.C && l < P.np) {
        if (MODE == 1) {
          // direction 0 of the natural layout: l = i_0, c = i_1 + np_1 i_2
          const int64_t i1 = c % P.npd[1], i2 = c / P.npd[1];
          if (l < P.nf[0] && i1 < P.nf[1] && i2 < P.nf[2]) {
            const int64_t g = (P.lo[0] + l) + P.N[0] * ((P.lo[1] + i1) + P.N[1] * (P.lo[2] + i2));
            v = P.r[g] * P.sv[g];
          }
        } else {
          v = P.X[c * P.np + l];
        }
      }
      rx[j] = v;
    }
  };
  fd_v4d acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; u++)
#pragma unroll
    for (int v = 0; v < 2; v++) acc[u][v] = (fd_v4d){0.0, 0.0, 0.0, 0.0};
  load(0);
  for (int l0 = 0; l0 < P.np; l0 += FD_KB) {
    __syncthreads();                      // (everyone is done with the last chunk)
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int e = tid + 256 * j;
      As[e >> 6][e & 63] = ra[j];
      Xs[e >> 5][e & 31] = rx[j];
    }
    __syncthreads();
    if (l0 + FD_KB < P.np) load(l0 + FD_KB);
#pragma unroll
    for (int k4 = 0; k4 < FD_KB / 4; k4++) {
      double a[2], b[2];
#pragma unroll
      for (int u = 0; u < 2; u++) a[u] = As[4 * k4 + lk][wi + 16 * u + lr];
#pragma unroll
      for (int v = 0; v < 2; v++) b[v] = Xs[wc + 16 * v + lr][4 * k4 + lk];
#pragma unroll
      for (int u = 0; u < 2; u++)
#pragma unroll
        for (int v = 0; v < 2; v++) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[v], acc[u][v], 0, 0, 0);
    }
  }
  // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int u = 0; u < 2; u++)
#pragma unroll
    for (int v = 0; v < 2; v++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int i = i0 + wi + 16 * u + lk + 4 * q;
        const int64_t c = c0 + wc + 16 * v + lr;
        if (i >= P.np || c >= P.C) continue;
        double val = acc[u][v][q];
        if (MODE == 2 || MODE == 3) {
          // direction d-1: i = i_{d-1}, c = i_0 + np_0 i_1
          const int64_t i0c = c % P.npd[0], i1c = c / P.npd[0];
          const bool inside = i < P.nf[P.d - 1] && i0c < P.nf[0] && (P.d < 3 || i1c < P.nf[1]);
          if (MODE == 2) {
            double s = P.coef[3] + P.coef[0] * (inside ? P.lam[0][i0c] : 0.0) + P.coef[P.d - 1] * P.lam[P.d - 1][i];
            if (P.d == 3) s += P.coef[1] * (inside ? P.lam[1][i1c] : 0.0);
            P.Y[(int64_t)i * P.C + c] = (inside && s > P.floor) ? val / s : 0.0;
          } else if (inside) {
            const int64_t g = P.d == 3 ? (P.lo[0] + i0c) + P.N[0] * ((P.lo[1] + i1c) + P.N[1] * (P.lo[2] + i))
                                       : (P.lo[0] + i0c) + P.N[0] * (P.lo[1] + i);
            P.z[g] = P.sv[g] * val;
          }
        } else {
          P.Y[(int64_t)i * P.C + c] = val;
        }
      }
}

// z_i = sv_i r_i for the dofs of the block outside its free box
__global__ void __launch_bounds__(256) k_fd_outside(const double *__restrict__ r, const double *__restrict__ sv,
                                                    double *__restrict__ z, int64_t N0, int64_t N1, int64_t N2, int64_t lo0,
                                                    int64_t lo1, int64_t lo2, int64_t n0, int64_t n1, int64_t n2) {
  const int64_t n = N0 * N1 * N2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride) {
    const int64_t a = g % N0, b = (g / N0) % N1, c = g / (N0 * N1);
    const bool inside = a >= lo0 && a < lo0 + n0 && b >= lo1 && b < lo1 + n1 && c >= lo2 && c < lo2 + n2;
    if (!inside) z[g] = sv[g] * r[g];
  }
}

// diag K: entry (r, r) of each row, 0 when absent (one wave per row, as the Jacobi set-up of the Krylov solvers)
__global__ void __launch_bounds__(256) k_fd_diag(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                 const double *__restrict__ val, int64_t nrows, double *__restrict__ diag) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < nrows; r += nwaves) {
    double d = 0.0;
    for (int64_t q = rowptr[r] + lane; q < rowptr[r + 1]; q += 64)
      if (col[q] == r) d = val[q];
    d = tg_wave_sum(d);
    if (lane == 0) diag[r] = d;
  }
}

struct fd_box_args {
  int d;
  int64_t N[3], lo[3];
  int nf[3];
  const double *dk[3], *dm[3];
  double coef[4];
};

// partials (one per workgroup, 4 streams) of <diag K, t_a> over the free box, t_a = prod_k (k == a ? dk_k : dm_k) for
// a < d and prod_k dm_k for a = 3
__global__ void __launch_bounds__(256) k_fd_fit(const double *__restrict__ diag, fd_box_args B, double *__restrict__ partial) {
  __shared__ double lds4[4];
  const int64_t n = (int64_t)B.nf[0] * B.nf[1] * B.nf[2];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const int i[3] = {(int)(t % B.nf[0]), (int)((t / B.nf[0]) % B.nf[1]), (int)(t / ((int64_t)B.nf[0] * B.nf[1]))};
    const int64_t g = (B.lo[0] + i[0]) + B.N[0] * ((B.lo[1] + i[1]) + B.N[1] * (B.lo[2] + i[2]));
    const double dg = diag[g];
    double m[3], k[3];
    for (int q = 0; q < 3; q++) {
      m[q] = q < B.d ? B.dm[q][i[q]] : 1.0;
      k[q] = q < B.d ? B.dk[q][i[q]] : 0.0;
    }
    s[0] += dg * (k[0] * m[1] * m[2]);
    s[1] += dg * (m[0] * k[1] * m[2]);
    s[2] += dg * (m[0] * m[1] * k[2]);
    s[3] += dg * (m[0] * m[1] * m[2]);
  }
  for (int a = 0; a < 4; a++) {
    const double v = tg_block_sum256(s[a], lds4);
    if (threadIdx.x == 0) partial[4 * blockIdx.x + a] = v;
  }
}

// sv on the free box: sqrt(diag P / diag K) (scaling) or 1; 1 / K_ii off the box
__global__ void __launch_bounds__(256) k_fd_scale(const double *__restrict__ diag, fd_box_args B, int scaling,
                                                  double *__restrict__ sv) {
  const int64_t n = B.N[0] * B.N[1] * B.N[2];
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a[3] = {g % B.N[0], (g / B.N[0]) % B.N[1], g / (B.N[0] * B.N[1])};
    bool inside = true;
    for (int q = 0; q < 3; q++) inside = inside && a[q] >= B.lo[q] && a[q] < B.lo[q] + B.nf[q];
    const double dg = diag[g];
    if (!inside) {
      sv[g] = dg != 0.0 ? 1.0 / dg : 1.0;
      continue;
    }
    if (!scaling) {
      sv[g] = 1.0;
      continue;
    }
    double m[3], k[3];
    for (int q = 0; q < 3; q++) {
      const int iq = (int)(a[q] - B.lo[q]);
      m[q] = q < B.d ? B.dm[q][iq] : 1.0;
      k[q] = q < B.d ? B.dk[q][iq] : 0.0;
    }
    const double dp = B.coef[0] * (k[0] * m[1] * m[2]) + B.coef[1] * (m[0] * k[1] * m[2]) + B.coef[2] * (m[0] * m[1] * k[2]) +
                      B.coef[3] * (m[0] * m[1] * m[2]);
    sv[g] = (dg > 0.0 && dp > 0.0) ? sqrt(dp / dg) : 1.0;
  }
}

static fd_box_args fd_args(const fd_block &b) {
  fd_box_args a;
  a.d = b.d;
  for (int q = 0; q < 3; q++) {
    a.N[q] = b.N[q];
    a.lo[q] = b.lo[q];
    a.nf[q] = b.nf[q];
    a.dk[q] = q < b.d ? b.dk[q] : nullptr;
    a.dm[q] = q < b.d ? b.dm[q] : nullptr;
  }
  for (int q = 0; q < 4; q++) a.coef[q] = b.coef[q];
  return a;
}

extern "C" int tg_fd_create(int64_t n, tg_fd_t *out) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(out && n > 0, "tg_fd_create: bad arguments");
  tg_fd_s *f = new tg_fd_s();
  f->n = n;
  *out = f;
  return 0;
}

extern "C" int tg_fd_destroy(tg_fd_t fd) {
  if (!fd) return 0;
  hipStreamSynchronize(g_tg.stream);
  for (auto &b : fd->blocks) tg_dfree(b.mem);
  tg_dfree(fd->diag);
  tg_dfree(fd->sv);
  tg_dfree(fd->w0);
  tg_dfree(fd->w1);
  delete fd;
  return 0;
}

extern "C" int tg_fd_add_block(tg_fd_t fd, int d, int64_t offset, const int64_t *shape, const int64_t *lo, const int64_t *hi,
                               const double *Q, const double *lam, const double *dk, const double *dm) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(fd && shape && lo && hi && Q && lam && dk && dm, "tg_fd_add_block: null argument");
  TG_REQUIRE(d == 2 || d == 3, "tg_fd_add_block: d must be 2 or 3");
  fd_block b;
  b.d = d;
  b.off = offset;
  int64_t total = 1, qsz = 0, lsz = 0, dsz = 0;
  for (int k = 0; k < d; k++) {
    TG_REQUIRE(0 <= lo[k] && lo[k] < hi[k] && hi[k] <= shape[k], "tg_fd_add_block: empty or out-of-range box");
    TG_REQUIRE(hi[k] - lo[k] <= 4096, "tg_fd_add_block: more than 4096 free functions in direction %d", k);
    b.N[k] = shape[k];
    b.lo[k] = lo[k];
    b.nf[k] = (int)(hi[k] - lo[k]);
    b.np[k] = (b.nf[k] + 15) / 16 * 16;
    total *= shape[k];
    qsz += 2 * (int64_t)b.np[k] * b.np[k];
    lsz += b.np[k];
    dsz += 2 * b.nf[k];
  }
  TG_REQUIRE(offset >= 0 && offset + total <= fd->n, "tg_fd_add_block: the block lies outside the matrix");
  TG_TRY(tg_dmalloc(&b.mem, qsz + lsz + dsz));
  // host staging: Q (nf x nf, row-major Q[l][i]) padded, and its transpose
  std::vector<double> h((size_t)(qsz + lsz + dsz), 0.0);
  int64_t pos = 0, qoff = 0, loff = 0, doff = 0;
  double *base = b.mem;
  for (int k = 0; k < d; k++) {
    const int nf = b.nf[k], np = b.np[k];
    double *qf = h.data() + pos, *qb = qf + (int64_t)np * np;
    for (int l = 0; l < nf; l++)
      for (int i = 0; i < nf; i++) {
        const double v = Q[qoff + (int64_t)l * nf + i];
        qf[(int64_t)l * np + i] = v;
        qb[(int64_t)i * np + l] = v;
      }
    b.Qf[k] = base + pos;
    b.Qb[k] = base + pos + (int64_t)np * np;
    pos += 2 * (int64_t)np * np;
    qoff += (int64_t)nf * nf;
  }
  for (int k = 0; k < d; k++) {
    for (int i = 0; i < b.nf[k]; i++) {
      h[pos + i] = lam[loff + i];
      b.lam_max[k] = std::max(b.lam_max[k], fabs(lam[loff + i]));
    }
    b.lam[k] = base + pos;
    pos += b.np[k];
    loff += b.nf[k];
  }
  for (int k = 0; k < d; k++) {
    for (int i = 0; i < b.nf[k]; i++) {
      h[pos + i] = dk[doff + i];
      h[pos + b.nf[k] + i] = dm[doff + i];
    }
    b.dk[k] = base + pos;
    b.dm[k] = base + pos + b.nf[k];
    pos += 2 * b.nf[k];
    doff += b.nf[k];
  }
  TG_CHECK_HIP(hipMemcpyAsync(b.mem, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, g_tg.stream));
  TG_CHECK_HIP(hipStreamSynchronize(g_tg.stream));
  if (b.box() > fd->wsize) {
    tg_dfree(fd->w0);
    tg_dfree(fd->w1);
    fd->w0 = fd->w1 = nullptr;
    fd->wsize = b.box();
    TG_TRY(tg_dmalloc(&fd->w0, fd->wsize));
    TG_TRY(tg_dmalloc(&fd->w1, fd->wsize));
  }
  fd->blocks.push_back(b);
  fd->ready = false;
  return 0;
}

// diag K and, per block, the 4 sums <diag K, t_a> (rhs[4 b + a]; a = 0..d-1 stiffness in direction a, 3 = mass)
extern "C" int tg_fd_fit(tg_fd_t fd, tg_csr_t k, double *rhs) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(fd && k && rhs, "tg_fd_fit: null argument");
  TG_REQUIRE_CANONICAL(k);
  TG_REQUIRE(k->nrows == fd->n && k->ncols == fd->n, "tg_fd_fit: the matrix is not %lld x %lld", (long long)fd->n,
             (long long)fd->n);
  const int64_t n = fd->n;
  if (!fd->diag) TG_TRY(tg_dmalloc(&fd->diag, n));
  if (k->diag_cache && k->diag_rows == n) {
    TG_CHECK_HIP(hipMemcpyAsync(fd->diag, k->diag_cache, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, g_tg.stream));
  } else {
    const unsigned jg = (unsigned)std::min<int64_t>(tg_cdiv(n, 4), (int64_t)g_tg.num_cu * 16);
    hipLaunchKernelGGL(k_fd_diag, dim3(jg), dim3(256), 0, g_tg.stream, k->rowptr, k->col, k->val, n, fd->diag);
  }
  double *part = g_tg.scratch;           // 4 * FD_FIT_BLOCKS
  std::vector<double> h(4 * FD_FIT_BLOCKS);
  for (size_t bi = 0; bi < fd->blocks.size(); bi++) {
    const fd_block &b = fd->blocks[bi];
    hipLaunchKernelGGL(k_fd_fit, dim3(FD_FIT_BLOCKS), dim3(256), 0, g_tg.stream, fd->diag + b.off, fd_args(b), part);
    TG_LAUNCH_CHECK();
    TG_CHECK_HIP(hipMemcpyAsync(h.data(), part, h.size() * sizeof(double), hipMemcpyDeviceToHost, g_tg.stream));
    TG_CHECK_HIP(hipStreamSynchronize(g_tg.stream));
    for (int a = 0; a < 4; a++) {
      double s = 0.0;
      for (int j = 0; j < FD_FIT_BLOCKS; j++) s += h[4 * j + a];
      rhs[4 * bi + a] = s;
    }
  }
  fd->fitted = true;
  fd->ready = false;
  return 0;
}

// coefficients per block (coef[4 b + a], a as in tg_fd_fit) and the scaling (1: D^-1/2, 0: none); needs tg_fd_fit before
extern "C" int tg_fd_set_coefficients(tg_fd_t fd, const double *coef, int scaling) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(fd && coef, "tg_fd_set_coefficients: null argument");
  TG_REQUIRE(fd->fitted, "tg_fd_set_coefficients: tg_fd_fit (diagonal of K) must come first");
  // every block's coefficients are checked before any is stored: a refusal leaves the previous set in force
  for (size_t bi = 0; bi < fd->blocks.size(); bi++) {
    const fd_block &b = fd->blocks[bi];
    double top = coef[4 * bi + 3];
    for (int a = 0; a < 4; a++) {
      const double c = (a < b.d || a == 3) ? coef[4 * bi + a] : 0.0;
      TG_REQUIRE(c >= 0.0 && c == c, "tg_fd_set_coefficients: negative or NaN coefficient");
      if (a < b.d) top += c * b.lam_max[a];
    }
    TG_REQUIRE(top > 0.0, "tg_fd_set_coefficients: every coefficient is zero");
  }
  if (!fd->sv) TG_TRY(tg_dmalloc(&fd->sv, fd->n));
  fd->ready = false;                     // (until every block's sv is written again)
  for (size_t bi = 0; bi < fd->blocks.size(); bi++) {
    fd_block &b = fd->blocks[bi];
    double top = coef[4 * bi + 3];
    for (int a = 0; a < 4; a++) b.coef[a] = (a < b.d || a == 3) ? coef[4 * bi + a] : 0.0;
    for (int k = 0; k < b.d; k++) top += b.coef[k] * b.lam_max[k];
    b.floor = 1e-13 * top;
    const int64_t nb = b.N[0] * b.N[1] * b.N[2];
    hipLaunchKernelGGL(k_fd_scale, dim3(tg_grid_1d(nb, 256)), dim3(256), 0, g_tg.stream, fd->diag + b.off, fd_args(b), scaling,
                       fd->sv + b.off);
    TG_LAUNCH_CHECK();
  }
  fd->ready = true;
  return 0;
}

// z = B r on the device (r and z are distinct vectors of fd->n entries)
static int tg_fd_apply_dev(tg_fd_s *fd, const double *r, double *z) {
  TG_REQUIRE(fd->ready, "tg_fd_apply: tg_fd_fit / tg_fd_set_coefficients must come first");
  for (const fd_block &b : fd->blocks) {
    fd_pass P;
    P.r = r + b.off;
    P.sv = fd->sv + b.off;
    P.z = z + b.off;
    P.d = b.d;
    for (int q = 0; q < 3; q++) {
      P.npd[q] = b.np[q];
      P.nf[q] = b.nf[q];
      P.lo[q] = b.lo[q];
      P.N[q] = b.N[q];
      P.lam[q] = q < b.d ? b.lam[q] : nullptr;
    }
    for (int q = 0; q < 4; q++) P.coef[q] = b.coef[q];
    P.floor = b.floor;
    const int64_t box = b.box();
    double *src = fd->w0, *dst = fd->w1;
    for (int pass = 0; pass < 2 * b.d; pass++) {
      const int k = pass % b.d;
      P.np = b.np[k];
      P.C = box / b.np[k];
      P.A = pass < b.d ? b.Qf[k] : b.Qb[k];
      P.X = src;
      P.Y = dst;
      const int64_t nwg = tg_cdiv(P.np, FD_MT) * tg_cdiv(P.C, FD_NT);
      TG_REQUIRE(nwg < (int64_t)1 << 31, "tg_fd_apply: box too large");
      if (pass == 0)
        hipLaunchKernelGGL(k_fd_mode<1>, dim3((unsigned)nwg), dim3(256), 0, g_tg.stream, P);
      else if (pass == b.d - 1)
        hipLaunchKernelGGL(k_fd_mode<2>, dim3((unsigned)nwg), dim3(256), 0, g_tg.stream, P);
      else if (pass == 2 * b.d - 1)
        hipLaunchKernelGGL(k_fd_mode<3>, dim3((unsigned)nwg), dim3(256), 0, g_tg.stream, P);
      else
        hipLaunchKernelGGL(k_fd_mode<0>, dim3((unsigned)nwg), dim3(256), 0, g_tg.stream, P);
      TG_LAUNCH_CHECK();
      std::swap(src, dst);
    }
    const int64_t nb = b.N[0] * b.N[1] * b.N[2];
    hipLaunchKernelGGL(k_fd_outside, dim3(tg_grid_1d(nb, 256)), dim3(256), 0, g_tg.stream, P.r, P.sv, P.z, b.N[0], b.N[1], b.N[2],
                       b.lo[0], b.lo[1], b.lo[2], (int64_t)b.nf[0], (int64_t)b.nf[1], (int64_t)b.nf[2]);
    TG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int tg_fd_apply(tg_fd_t fd, tg_vec_t r, tg_vec_t z) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(fd && r && z, "tg_fd_apply: null argument");
  TG_REQUIRE(r->n == fd->n && z->n == fd->n, "tg_fd_apply: vector length != %lld", (long long)fd->n);
  TG_REQUIRE(r->d != z->d, "tg_fd_apply: r and z must be different vectors");
  return tg_fd_apply_dev(fd, r->d, z->d);
}

extern "C" int tg_krylov_solve_fd(tg_csr_t k, tg_fd_t fd, tg_vec_t b, tg_vec_t x, double rtol, double atol, int maxit,
                                  int flags, int *iters, double *resnorm, int *status) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(k && fd && b && x && iters && resnorm && status, "null argument to tg_krylov_solve_fd");
  TG_REQUIRE_CANONICAL(k);
  TG_REQUIRE(k->nrows == k->ncols && k->nrows == fd->n, "tg_krylov_solve_fd: K is not %lld x %lld", (long long)fd->n,
             (long long)fd->n);
  TG_REQUIRE(b->n == k->nrows && x->n == k->nrows, "tg_krylov_solve_fd: vector length != rows of K");
  tg_ksp_op op;
  TG_TRY(op.init(k, nullptr, true, (flags & TG_KSP_SYMMETRIC) != 0));
  return tg_pcg_host(op, [fd](const double *r, double *u) { return tg_fd_apply_dev(fd, r, u); }, b, x, rtol, atol, maxit,
                     (flags & TG_KSP_NONZERO_GUESS) ? 1 : 0, iters, resnorm, status);
}
