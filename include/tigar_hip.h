/*
 * tigar_hip.h -- C-ABI of libtigar_hip.so: the MI355X (gfx950) implementation of the
 * tIGAr extraction hot path.  Loaded from Python with ctypes (tigar_amd/_lib.py).
 *
 * The reference has no C boundary on this path: its seams are Python method contracts
 * (SURVEY.md section 8b).  Each entry point below names the reference interface it
 * replaces (paths relative to the reference root).
 *
 * Conventions: every call returns 0 on success, non-zero on failure (message via
 * tg_last_error()); device objects are opaque handles with explicit *_destroy; host
 * arrays are plain pointers + sizes; row pointers / sizes are int64, column indices
 * int32 (INDEX_TYPE='int32', tIGAr/common.py:43), values fp64.  Calls on one device are
 * serialised on the library's stream; the library is not thread-safe.
 */
#ifndef TIGAR_HIP_H
#define TIGAR_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct tg_csr_s *tg_csr_t;   /* device-resident CSR row block            */
typedef struct tg_vec_s *tg_vec_t;   /* device-resident fp64 vector              */
typedef struct tg_ptap_s *tg_ptap_t; /* symbolic plan of K = M^T A M             */
typedef struct tg_cellplan_s *tg_cellplan_t; /* K = M^T A M on a cell-local FE space: dense blocks per cell */
typedef struct tg_comm_s *tg_comm_t; /* RCCL communicator + z-slab descriptor    */
typedef struct tg_fd_s *tg_fd_t;     /* fast diagonalization preconditioner (csrc/tg_fd.hip) */

/* ---- runtime ------------------------------------------------------------------ */
int tg_init(int device);                   /* binds the HIP device, creates the stream */
int tg_shutdown(void);
const char *tg_last_error(void);
int tg_sync(void);                         /* hipStreamSynchronize on the library stream */
/* Second stream.  Every call of the library works on the CURRENT stream (0 after tg_init).
 * tg_stream_set(1) makes a second stream current: what a caller enqueues there (e.g. the FE input of the
 * next sub-slab -- in the reference the FE assembly is dolfin's job, tIGAr/common.py:1206-1220) runs
 * beside the work on stream 0.  tg_stream_wait(a, b): stream a waits for everything enqueued so far on
 * stream b (device side, no host synchronisation); the caller orders the hand-over of objects
 * between the streams with it.  Freed device blocks are re-used across the streams safely (events).
 * tg_sync synchronises the current stream only. */
int tg_stream_set(int stream);
int tg_stream_wait(int waiter, int waited);
int tg_device_info(char *name, int name_len, int *num_cu, int64_t *hbm_bytes);
int tg_mem_info(int64_t *free_bytes, int64_t *total_bytes);
int tg_pool_trim(void);
/* caching allocator statistics: bytes / blocks held free in the pool, blocks handed out */
int tg_pool_stats(int64_t *pooled_bytes, int64_t *pooled_blocks, int64_t *live_blocks);                    /* releases the caching allocator's free blocks */
/* HIP-event timers on the library's stream (bench.py roofline measurement). */
int tg_timer_start(int slot);
int tg_timer_stop(int slot, double *ms);   /* synchronises; elapsed ms since start(slot) */

/* Per-kernel accounting filled by the library while it runs (HIP events on the library's
 * stream, resolved at the next host sync).  slot 0: the SpMV inside tg_krylov_solve; slot 1 (count only): those of
 * them whose halo-free rows were computed while the halo exchange with the neighbour ranks was under way; slot 2 (count
 * only): sliced copies (tg_spmv_sell / Krylov solves) built on the slice classes of an earlier matrix with the same
 * pattern instead of a new classification; slot 3 (count only): x passes of the tensor-pattern PtAP that took the FE
 * matrix' pattern from its certificate (written by tg_kron_sum_csr) instead of verifying every column index; slot 4 (count only): host waits
 * (hipStreamSynchronize / transport calls) the device communicator needed inside halo exchanges and all-reduces -- 0 for
 * RCCL and for the IPC communicator, whose exchanges are enqueued only; slot 5 (count only): final stages of the
 * tensor-pattern PtAP (tg_tensor_zstage, tg_tensor2_ptap) that delivered rows of K -- "the line walks ran"; slot 6: CG /
 * GMRES solves that ran as ONE persistent kernel (small systems, csrc/tg_krylov_small.hip): count, and the time of those kernels
 * (their products are also counted in slot 0, with the kernel time spread over them -- an iteration, not a product);
 * slot 7 (count only): CG solves whose products ran on the half-storage copy of csrc/tg_symgrid.hip; slot 8 (count only):
 * direct solves (tg_lu_solve) that ran as a banded Cholesky factorisation (csrc/tg_chol.hip: symmetric positive definite K). */
enum { TG_PROF_KSP_SPMV = 0, TG_PROF_KSP_OVERLAPPED = 1, TG_PROF_SELL_SHAPE_REUSED = 2, TG_PROF_PTAP_CERTIFIED = 3,
       TG_PROF_COMM_HOST_WAITS = 4, TG_PROF_PTAP_TENSOR_WALKS = 5, TG_PROF_KSP_PERSISTENT = 6, TG_PROF_KSP_SYMGRID = 7,
       TG_PROF_LU_CHOLESKY = 8, TG_PROF_NSLOTS = 9 };
int tg_prof_reset(void);
int tg_prof_get(int slot, double *total_ms, int64_t *count);

/* ---- vectors ------------------------------------------------------------------ */
int tg_vec_create(int64_t n, tg_vec_t *out);               /* zero-initialised */
int tg_vec_create_uninit(int64_t n, tg_vec_t *out);        /* contents undefined: for outputs a kernel overwrites entirely
                                                              (PETSc's VecDuplicate leaves the values unset as well) */
int tg_vec_destroy(tg_vec_t v);
int tg_vec_size(tg_vec_t v, int64_t *n);
int tg_vec_upload(tg_vec_t v, const double *host, int64_t n);
int tg_vec_download(tg_vec_t v, double *host, int64_t n);
int tg_vec_fill(tg_vec_t v, double a);
int tg_vec_copy(tg_vec_t dst, tg_vec_t src);
int tg_vec_copy_range(tg_vec_t dst, int64_t dst_off, tg_vec_t src, int64_t src_off, int64_t n);
int tg_vec_axpy(tg_vec_t y, double a, tg_vec_t x);          /* y += a x */
int tg_vec_dot(tg_vec_t x, tg_vec_t y, double *out);        /* deterministic two-stage */
int tg_vec_pointwise_mult(tg_vec_t w, tg_vec_t x, tg_vec_t y);   /* w = x .* y (VecPointwiseMult) */
int tg_vec_pointwise_divide(tg_vec_t w, tg_vec_t x, tg_vec_t y); /* w = x ./ y (VecPointwiseDivide) */
/* GenericVector::norm: kind 0 = "l1", 1 = "l2", 2 = "linf" (tIGAr/common.py:1330 norm(MTb)) */
int tg_vec_norm(tg_vec_t x, int kind, double *out);
/* as_backend_type(MTb).vec().setValues(zeroDofs, 0)  -- tIGAr/common.py:1154-1158 */
int tg_vec_zero_entries(tg_vec_t y, const int32_t *dofs, int64_t n);
/* same for a slab-local vector holding global entries [g0, g0 + size(y)) */
int tg_vec_zero_entries_offset(tg_vec_t y, const int32_t *dofs, int64_t n, int64_t g0);
/* separable load b[(a,b,c)] = scale * b0[a]*b1[b]*b2[c] (synthetic input) */
int tg_vec_tensor3(tg_vec_t out, int d, const double *const *b1d, const int64_t *n,
                   double scale, int64_t row0, int64_t row1);

/* ---- CSR objects ---------------------------------------------------------------- */
int tg_csr_from_host(int64_t nrows, int64_t ncols, const int64_t *rowptr,
                     const int32_t *col, const double *val, tg_csr_t *out);
int tg_csr_dims(tg_csr_t m, int64_t *nrows, int64_t *ncols, int64_t *nnz);
int tg_csr_download(tg_csr_t m, int64_t *rowptr, int32_t *col, double *val);
/* rows [r0,r1) only: rowptr_out[r1-r0+1] relative to the first entry; col/val NULL = sizes only (two-call
 * protocol).  PETSc counterpart: MatGetRow on a row sample of MTAM (tIGAr/common.py:1194-1204) [ext]. */
int tg_csr_download_rows(tg_csr_t m, int64_t r0, int64_t r1, int64_t *rowptr_out, int32_t *col, double *val,
                         int64_t cap);
int tg_csr_destroy(tg_csr_t m);
/* explicit M^T (the reference's FORM_MT switch, tIGAr/common.py:84,358-360);
 * deterministic: rows of M^T sorted by FE row index. */
int tg_csr_transpose(tg_csr_t m, tg_csr_t *out);
/* IGA dof permutation (tIGAr/common.py:407-433 applyPermutation, 1583-1665 generatePermutation).
 * tg_partition_mode: mt = transposed extraction pattern (rows = IGA dofs, columns = FE rows); fe_owner[j] (host, one
 * entry per FE row, 0 <= owner < world) = the rank owning FE row j; owner_out[i] (host) = the rank owning the most FE
 * rows of dof i's support, the lowest such rank on a tie (scipy.stats.mode), 0 for an empty row.
 * tg_csr_permute_columns: copy of m with column c renamed new_of_old[c] (host, ncols entries, a permutation), rows
 * re-sorted: MatPermute with identity rows. */
/* Field blocks of a matrix on a mixed space whose dofs are numbered field after field (the FE matrices of
 * EqualOrderSpline(nFields > 1), tIGAr/common.py:1891-1914): tg_csr_block cuts out rows [r0, r1) x columns [c0, c1)
 * (columns renumbered from 0); tg_csr_from_blocks puts nf x nf blocks together (equal row counts along a block row, equal column
 * counts down a block column: the fields of a FieldListSpline differ in size), blocks[i * nf + j] at block
 * row i, block column j.  Used to run the scalar tensor-pattern PtAP block by block. */
/* C = A + B on the union of the two patterns (MatAXPY, DIFFERENT_NONZERO_PATTERN [ext]); ascending columns. */
int tg_csr_add(tg_csr_t a, tg_csr_t b, tg_csr_t *out);
int tg_csr_block(tg_csr_t a, int64_t r0, int64_t r1, int64_t c0, int64_t c1, tg_csr_t *out);
/* A copy of `a` (same shape) without the entries whose column c has keep[c] == 0 (host array, ncols bytes).  Used to split
 * M^T A M by residue classes of the columns when a row of the product exceeds the per-row tables of the general kernels
 * (3-D patches of degree >= 5; tIGAr/common.py:1194-1195 has no degree limit). */
int tg_csr_select_columns(tg_csr_t a, const uint8_t *keep, tg_csr_t *out);
int tg_csr_from_blocks(int nf, const tg_csr_t *blocks, tg_csr_t *out);
/* a = d + r on a cell-local FE space (nodes numbered cell after cell, b per cell): d = the entries of the diagonal b x b cell
 * blocks, r = all others, both with a's shape.  100: some row does not hold all b entries of its own block (a is not "what
 * dolfin assembles on the mesh of disconnected cells" plus extra couplings).  The matrix of demos/kl-shell-svk/reef-knot.py:
 * 455-467 -- a T-spline stiffness matrix with contact terms added by hand, the reason extractMatrix takes any A
 * (tIGAr/common.py:1175) -- splits this way: d goes through the cell-block product (tg_cellplan_ptap), r through the general
 * kernels, the results are added on the union pattern (tg_csr_add). */
int tg_csr_split_cells(tg_csr_t a, int b, tg_csr_t *d_out, tg_csr_t *r_out);
/* out row r = row rows[r] of a (host index array; any selection or order, repetitions allowed), columns untouched */
int tg_csr_gather_rows(tg_csr_t a, const int64_t *rows, int64_t n, tg_csr_t *out);
int tg_partition_mode(tg_csr_t mt, const int32_t *fe_owner, int world, int32_t *owner_out);
int tg_csr_permute_columns(tg_csr_t m, const int32_t *new_of_old, tg_csr_t *out);
/* fallback for arbitrary AbstractScalarBasis plug-ins (seam b-2, tIGAr/common.py:1683-1692):
 * rows fed as (row, col, val) triplets from the host loop of generateM; applies the
 * abs(v) > eps filter of tIGAr/common.py:1569, INSERT semantics (last wins), sorts columns. */
int tg_csr_from_triplets(int64_t nrows, int64_t ncols, int64_t nt, const int64_t *rows,
                         const int32_t *cols, const double *vals, double eps, tg_csr_t *out);

/* ---- extraction-operator build (generateM) ------------------------------------- */
/* One univariate B-spline direction of a tensor-product basis (BSpline1,
 * tIGAr/BSplines.py:164-351) plus the FE node coordinates along that direction. */
typedef struct {
  int32_t p;              /* degree                                              */
  int32_t nknots;         /* len(knots)                                          */
  const double *ghost;    /* ghostKnots, length nknots + 2*(p+1)  (:204-212)     */
  int32_t mult_first;     /* multiplicities[0]                                   */
  int32_t mult_last;      /* multiplicities[-1]                                  */
  int32_t ncp;            /* number of basis functions (:273-277)                */
  int64_t nnodes;         /* FE nodes along this direction                       */
  const double *nodes;    /* their parametric coordinates (host)                 */
} tg_dir_t;

/* Replaces AbstractCoordinateChartSpline.generateM / generateM_control
 * (tIGAr/common.py:1460-1578) + BSpline.getNodesAndEvals (tIGAr/BSplines.py:450-503)
 * + basisFuncsInner (tIGAr/BSplines.py:73-120) for BSpline bases on the implicit
 * tensor FE node grid.  Rows = nodes in lexicographic order (direction 0 fastest),
 * restricted to [row0,row1) (a z-slab); column = i + j*ncp0 + k*ncp0*ncp1 + col_offset;
 * entries with fabs(v) > eps kept; columns sorted.  ncols = total columns of the block. */
int tg_extract_csr_tensor(int d, const tg_dir_t *dirs, int32_t col_offset, int64_t ncols,
                          double eps, int64_t row0, int64_t row1, tg_csr_t *out);
/* The explicit transpose M^T of the same operator (the reference's FORM_MT object,
 * tIGAr/common.py:84,358-360), written directly: rows = spline dofs [dof0,dof1) of this field,
 * columns = fe_row_offset + lexicographic FE node index; bit-identical to transposing
 * tg_extract_csr_tensor's result. */
int tg_extract_csr_tensor_t(int d, const tg_dir_t *dirs, int64_t fe_row_offset, int64_t fe_rows_total,
                            double eps, int64_t dof0, int64_t dof1, tg_csr_t *out);
/* Matrix-free y = M x for the same operator (rows [row0,row1), x holding the columns
 * [x_col0, x_col0+size(x))): prolongation u = M*U (tIGAr/common.py:1259) without M in memory. */
int tg_extract_apply_tensor(int d, const tg_dir_t *dirs, int32_t col_offset, double eps, int64_t row0,
                            int64_t row1, tg_vec_t x, int64_t x_col0, tg_vec_t y);
/* Same with explicit node coordinates x[nrows*d] (dolfin-supplied / DG nodes). */
int tg_extract_csr_points(int d, const tg_dir_t *dirs, int32_t col_offset, int64_t ncols,
                          double eps, const double *x, int64_t nrows, tg_csr_t *out);
/* vertical concatenation of row blocks (multi-field M: one block per field) */
int tg_csr_vstack(int nblocks, const tg_csr_t *blocks, tg_csr_t *out);
/* The same stacked matrix WITHOUT copying entries: a loose-row view whose rows point into the
 * blocks' own col/val arrays (20 B per row are written instead of 12 B per entry).  The blocks
 * (canonical or loose-row) must outlive the view; accepted where loose-row matrices are. */
int tg_csr_vstack_view(int nblocks, const tg_csr_t *blocks, tg_csr_t *out);
/* Incremental vstack: K is assembled slab by slab into ONE allocation (no second copy of a 70 GB
 * matrix): create with an nnz capacity estimate, append row blocks in order (the block's arrays
 * are copied device-to-device; the capacity grows geometrically if the estimate was short),
 * finish to obtain the CSR object. */
typedef struct tg_csr_builder_s *tg_csr_builder_t;
int tg_csr_builder_create(int64_t nrows_total, int64_t ncols, int64_t nnz_capacity, tg_csr_builder_t *out);
int tg_csr_builder_append(tg_csr_builder_t b, tg_csr_t block);
int tg_csr_builder_finish(tg_csr_builder_t b, tg_csr_t *out);   /* destroys the builder */
int tg_csr_builder_destroy(tg_csr_builder_t b);                 /* abandons an unfinished builder */
/* 1-D evaluation only (device twin of BSpline1.getKnotSpan/getNodes/basisFuncs):
 * idx[n*(p+1)], val[n*(p+1)] in the reference's order (span-p .. span). */
int tg_eval_basis_1d(const tg_dir_t *dir, const double *u, int64_t n, int32_t *span,
                     int32_t *idx, double *val);

/* ---- extraction application ------------------------------------------------------ */
/* y = A x   (prolongation u = M*U, tIGAr/common.py:1259; K*p inside the Krylov solve).
 * x must cover columns [col_base, col_base + size(x)). */
int tg_spmv(tg_csr_t a, tg_vec_t x, tg_vec_t y);
/* same with x covering only the columns [x_col0, x_col0 + size(x)) of a row block whose
 * entries all fall in that range (z-slab pieces of M, M^T, K) */
int tg_spmv_offset(tg_csr_t a, tg_vec_t x, int64_t x_col0, tg_vec_t y);
/* Sliced, pattern-compressed copy of the VALUES of `a` for repeated products (tg_sell.hip).  The
 * Krylov solvers build and drop it themselves for every solve (the K p of KSP on PETSc AIJ,
 * tIGAr/common.py:1255-1258); this entry point keeps one on the matrix so that tg_spmv / tg_spmv_offset
 * use it as well.  It is a snapshot: request it again after changing values.  Stencil-like matrices
 * (K = M^T A M of tensor-product patches) are accepted -- rows in slices of 64, one sorted union of
 * column offsets col - row per slice, values as dense [offsets][64] blocks, 8 B instead of 12 B per
 * entry and no gather -- others are declined and keep the CSR kernel (nclasses = 0).  Rows are summed
 * sequentially in ascending column order (PETSc's order); padded positions add +0.0.
 * enable = 0 drops the copy.  nclasses / padded (may be NULL): dictionary size, doubles stored. */
int tg_spmv_sell(tg_csr_t a, int enable, int *nclasses, int64_t *padded);
/* Half-storage product (csrc/tg_symgrid.hip) -- what the CG solve of tg_krylov_solve uses for its K p when K is a
 * SYMMETRIC box stencil of radius 1..3 on a 3-D grid held by one rank (K = M^T A M of one scalar field on a 3-D patch;
 * the reference hands K to PETSc's KSPCG, tIGAr/common.py:1255-1258, whose premise is a symmetric operator): the diagonal
 * and the entries above it are stored once (172 of 343 per row for p = 3) and used for the row and for the transposed
 * entry; the scatter goes through a ring of LDS windows per (x, y) patch walked along z, deterministically (no global
 * atomics).  `a` is the whole matrix (row0 = 0) or the block of rows [row0, row0 + nrows) a rank holds -- whole planes of
 * the grid, all columns: rows in its first planes also take their entries below the block from the CSR arrays (the
 * previous rank stores those as ITS upper triangle), what is scattered beyond the block is dropped; the solve does this
 * per z slab after the usual halo exchange of the vector.  This entry point plans the copy for `a`, checks it against the
 * CSR product on a pseudo-random vector, and, with x (all columns) and y given, computes y = a x with it.  *accepted = 0:
 * `a` has no such structure or is not symmetric (nothing is computed).  value_bytes / staging_bytes (may be NULL): bytes of
 * K one product reads / size of the window staging. */
int tg_spmv_symgrid(tg_csr_t a, int64_t row0, tg_vec_t x, tg_vec_t y, int *accepted, int64_t *value_bytes,
                    int64_t *staging_bytes);
/* The same, with the account of the delta-coded values (TIGAR_SYMGRID_DELTA, default on: the values of a scalar plan as
 * int16 distances, in 64-bit integer arithmetic, from the fp64 blocks of one reference plane -- restored bit for bit in the
 * product; a matrix whose planes are unlike each other keeps fp64 values).  value_bytes stays the fp64 half-storage figure.
 * info[12]: [0] 1 = delta-coded, [1] parts (32 rows of a sub-step; radius 4: 16) a product reads, [2] parts stored as
 * deltas, [3] reference plane (global index: the plane of the block nearest n2 / 2), [4] template bytes, [5] delta bytes,
 * [6] pool bytes in use (fp64 parts that did not fit), [7] pool capacity in parts, [8] largest distance of a part that
 * fits, [9] value bytes one product reads from HBM, [10] bytes the values occupy, [11] z chunks of the plan. */
int tg_spmv_symgrid_delta(tg_csr_t a, int64_t row0, tg_vec_t x, tg_vec_t y, int *accepted, int64_t *value_bytes,
                          int64_t *staging_bytes, int64_t *info);
/* How the scalar half-storage product of radius P (1..4; coded: the delta-coded plan's kernel, else the plain one) fills
 * the chip -- out[8]: [0] workgroups (one wave each) a CU holds, as hipOccupancyMaxActiveBlocksPerMultiprocessor reports for
 * that kernel, [1] its static LDS bytes, [2] places = [0] x the CUs, [3] the z chunks the plan builder chooses for a whole
 * grid of n0 x n1 x n2 points on those places (TIGAR_SYMGRID_CHUNKS overrides it here as it does there; 0 when n0 <= 0),
 * [4], [5] the largest patch (points in x, y), [6] CUs, [7] 0.  Host arithmetic and two runtime queries: no plan is built. */
int tg_symgrid_occupancy(int P, int coded, int n0, int n1, int n2, int64_t *out);
/* The scalar half-storage plan this process built last (by tg_spmv_symgrid* or by a CG solve) -- out[4]: [0] its radius P
 * (0: none built yet), [1] its z chunks, [2] the places its builder chose them for, [3] the workgroups per CU behind [2]
 * (the fewer of the plain and the delta-coded kernel's when the coding was tried, else the plain kernel's). */
int tg_symgrid_last_plan(int64_t *out);
/* Y = A X for k <= 4 right-hand sides (cpFuncs = M_control * P, tIGAr/common.py:367-380);
 * X, Y are column-major host arrays. */
int tg_spmm_host(tg_csr_t a, const double *X, int k, double *Y);
/* multTranspose / extractVector (tIGAr/common.py:97-109,1142-1160): y = M^T b using the
 * explicit transpose mt (scatter-free, deterministic). */
int tg_spmv_t(tg_csr_t mt, tg_vec_t b, tg_vec_t y);

/* extractMatrix (tIGAr/common.py:1176-1204): K = M^T A M (PETSc MatPtAP [ext]).
 * symbolic: pattern + plan; numeric: values (+ optional fused zeroRowsColumns).
 * Row-block form: computes K rows [i0,i1) from mt rows [i0,i1) (local rows of `mt`
 * start at global row mt_row0), A rows starting at a_row0, M rows starting at m_row0. */
int tg_ptap_symbolic(tg_csr_t a, int64_t a_row0, tg_csr_t m, int64_t m_row0, tg_csr_t mt,
                     int64_t mt_row0, tg_ptap_t *plan);
int tg_ptap_numeric(tg_ptap_t plan, tg_csr_t a, tg_csr_t m, tg_csr_t mt,
                    const int32_t *zero_dofs, int64_t nzero, double diag, tg_csr_t *k_out);
int tg_ptap_destroy(tg_ptap_t plan);
/* Which kernels tg_ptap_symbolic plans for: 0 = chosen from the operands (default), 1 = two row-wise Gustavson products
 * with one wave per row (csrc/tg_ptap_wave.hip: faster for long operand rows, 3-D p >= 3), 2 = the fused
 * workgroup-per-row kernel (csrc/tg_ptap.hip).  The result is the same matrix either way (MatPtAP, tIGAr/common.py:1194-1195);
 * a caller that streams the product in row blocks with overlapping operands states its preference here.  Returns the
 * previous setting. */
int tg_ptap_prefer(int kernels);
/* extractMatrix on a CELL-LOCAL FE space (the meshes of disconnected cells of tIGAr/RhinoTSplines.py:195-240 and
 * tIGAr/BSplines.py:800-860: b nodes per cell, numbered cell after cell), where an assembled A is block diagonal with one
 * dense b x b block per cell: K = sum_c S_c^T (M_c^T A_c M_c) S_c -- dense element matrices out of LDS, merged into K by
 * the look-up stage of the wave kernels.  The plan depends on M only (host-built: md [ncell][b][nfmax] dense rows of M per
 * cell over the cell's function list fl [ncell][nfmax] (nf[c] of them used), incidence: row i -> rows c * nfmax + q of
 * the element matrices holding function i, borrowed for the plan's lifetime; max_k / mean_k: row lengths of K).
 * tg_cellplan_ptap returns 100 when `a` is not such a block-diagonal matrix (use tg_ptap_*). */
int tg_cellplan_create(int64_t ncell, int b, int nfmax, int64_t ncols, const double *md_host, const int32_t *fl_host,
                       const int32_t *nf_host, tg_csr_t incidence, int max_k, double mean_k, tg_cellplan_t *out);
int tg_cellplan_ptap(tg_cellplan_t plan, tg_csr_t a, const int32_t *zero_dofs, int64_t nzero, double diag, tg_csr_t *k_out);
int tg_cellplan_destroy(tg_cellplan_t plan);
/* extractMatrix for ARBITRARY sparse operands on a CONNECTED mesh (cells share nodes: what dolfin assembles on a Q_p / P_p mesh,
 * tIGAr/common.py:1194-1195 with an M that is not used as a Kronecker product), csrc/tg_elemsplit.hip.  A = sum_c R_c^T A_c R_c
 * for ANY splitting of its entries over the cells that hold both nodes, hence K = sum_c (R_c M)^T A_c (R_c M): dense products
 * per cell, merged into K by stored places.  Everything runs on the device; the input besides the CSR operands is the cells'
 * node lists (dolfin: V.dofmap().cell_dofs(c)).
 * tg_cells_t: node lists [ncell][b] (b <= 128), from a host array or, for this package's stand-in of the FE space (continuous
 * Q_p on a tensor-product grid of nodes, direction 0 fastest), generated on the device for a box of elements.
 * tg_elemplan_create: the plan for the cells [own0, own1) of `cells` -- listed cells outside that range only take part in the
 * ownership rule (an entry of A belongs to the FIRST listed cell that holds both its nodes), so a mesh can be worked off in
 * chunks whose K are added.  m holds the rows [m_row0, ...) of M (global columns) of all nodes of the own cells; `cells` and `m`
 * are borrowed for the plan's lifetime.  Status 100: the cells do not qualify (more than 128 functions in a cell, a function in
 * more than 128 cells).
 * tg_elemplan_ptap: rows [dof0, dof1) (tg_elemplan_info) of sum over the own cells, global columns, MatZeroRowsColumns applied
 * when zero_dofs is given.  a holds the rows [a_row0, ...) of A; every entry of the rows [check_row0, check_row1) must couple two
 * nodes of a listed cell, else status 100 (a coupling added by hand, demos/kl-shell-svk/reef-knot.py:455-467: take tg_ptap_*).
 * The pattern of K and the places are found on the first product and kept by the plan. */
typedef struct tg_cells_s *tg_cells_t;
typedef struct tg_elemplan_s *tg_elemplan_t;
int tg_cells_from_host(const int32_t *nodes_host, int64_t ncell, int b, tg_cells_t *out);
int tg_cells_from_grid(int d, const int64_t *nodes_per_dir, int degree, const int64_t *elem_lo, const int64_t *elem_hi,
                       tg_cells_t *out);
int tg_cells_dims(tg_cells_t cells, int64_t *ncell, int *b);
int tg_cells_download(tg_cells_t cells, int32_t *nodes_host);
int tg_cells_destroy(tg_cells_t cells);
int tg_elemplan_create(tg_cells_t cells, int64_t own0, int64_t own1, tg_csr_t m, int64_t m_row0, tg_elemplan_t *out);
int tg_elemplan_info(tg_elemplan_t plan, int64_t *dof0, int64_t *dof1, int *nfmax, int *ninc_max, int64_t *k_nnz);
int tg_elemplan_ptap(tg_elemplan_t plan, tg_csr_t a, int64_t a_row0, int64_t check_row0, int64_t check_row1,
                     const int32_t *zero_dofs, int64_t nzero, double diag, tg_csr_t *k_out);
int tg_elemplan_destroy(tg_elemplan_t plan);
/* The same product for a matrix that holds its dense cell blocks PLUS couplings outside them (contact / penalty terms added by
 * hand to a T-spline matrix: demos/kl-shell-svk/reef-knot.py:455-467, the reason extractMatrix takes any A, tIGAr/common.py:
 * 1175): k_out = M^T D M from the blocks D read in place (no copy of A), r_out = the remainder A - D with A's shape, whose
 * product goes through the general kernels and is added on the union pattern (tg_csr_add).  100: some row lacks entries of
 * its own block.  No boundary conditions here (MatZeroRowsColumns follows the sum). */
int tg_cellplan_ptap_extras(tg_cellplan_t plan, tg_csr_t a, tg_csr_t *k_out, tg_csr_t *r_out);
/* The rows of `a` that hold entries, ascending, into rows_host[0 .. min(*count, cap)); cap = 0 asks for the count only. */
int tg_csr_nonempty_rows(tg_csr_t a, int64_t cap, int64_t *rows_host, int64_t *count);

/* K = R^T K_u R for a 0/1 matrix R with ONE entry per row, MatZeroRowsColumns (tIGAr/common.py:1196-1204) fused, on a PLAN:
 * after the tensor line walks ran on the unwrapped space of a patch with periodic directions (tIGAr/BSplines.py:204-212,
 * 310-319: `% ncp` in getNodes; R = which unwrapped function is which spline function) the rows of K_u that R identifies are
 * added and the columns renamed.  tg_foldplan_create takes the pattern of K from a first product made with the general
 * kernels (tg_ptap_numeric(K_u, R, R^T)) and stores the place of every entry of K_u in its row of K; tg_foldplan_apply then
 * is one pass over K_u without any look-up (status 100: K_u has another pattern than the plan's -- checksum of its row
 * pointer and columns -- or a row of K too long for the 16-bit places: use the general kernels).  ku: rows ku_row0 ... of
 * K_u with global (unwrapped) columns; r: all rows of R; rt: the rows rt_row0 ... of R^T = the rows of K (borrowed by the
 * plan: it must outlive it). */
typedef struct tg_foldplan_s *tg_foldplan_t;
int tg_foldplan_create(tg_csr_t ku, int64_t ku_row0, tg_csr_t r, tg_csr_t rt, int64_t rt_row0, tg_csr_t k, tg_foldplan_t *out);
int tg_foldplan_apply(tg_foldplan_t plan, tg_csr_t ku, const int32_t *zero_dofs, int64_t nzero, double diag, tg_csr_t *k_out);
int tg_foldplan_destroy(tg_foldplan_t plan);
/* extractMatrix when the extraction operator is a Kronecker product (tensor B-splines): one
 * contraction stage  out = P^T cur P  with P = (x)_k F_k, F_k = the 1-D matrix of direction k
 * (n x m CSR + its transpose, host pointers) or the identity (rowptr == NULL).  `cur` is an
 * arbitrary sparse row block on the tensor index space dims_in (rows starting at cur_row0,
 * global columns); rows [out_row0,out_row1) of the result are produced.  Accumulates in a dense
 * LDS box addressed directly (no hashing).  Returns 100 when the box would not fit in LDS --
 * use tg_ptap_symbolic/numeric with explicit operators instead. */
typedef struct {
  int64_t n, m;                 /* F is n x m                                   */
  const int32_t *rowptr;        /* n+1, NULL = identity (direction not contracted) */
  const int32_t *col;
  const double *val;
  const int32_t *t_rowptr;      /* transpose, m+1                               */
  const int32_t *t_col;
  const double *t_val;
} tg_kron1d_t;
int tg_ptap_kron(tg_csr_t cur, int64_t cur_row0, int d, const int64_t *dims_in, const tg_kron1d_t *fac,
                 int64_t out_row0, int64_t out_row1, const int32_t *zero_dofs, int64_t nzero, double diag,
                 tg_csr_t *out);
/* Intermediate stage of a direction-by-direction product (no boundary conditions).  The result
 * is a LOOSE-ROW matrix: its rows lie where the kernel reserved space for them (the row-reorder copy
 * is skipped); it may only be passed on to tg_ptap_kron / tg_ptap_kron_stage (as `cur`),
 * tg_csr_vstack (with other loose-row blocks), tg_csr_compact, tg_csr_dims, tg_csr_download and
 * tg_csr_destroy -- every other entry point rejects it. */
int tg_ptap_kron_stage(tg_csr_t cur, int64_t cur_row0, int d, const int64_t *dims_in,
                       const tg_kron1d_t *fac, int64_t out_row0, int64_t out_row1, tg_csr_t *out);
/* Last stage with the result appended to a slab-wise builder of K (tg_csr_builder_*): the rows
 * [out_row0,out_row1) must be the next rows the builder expects; saves the block allocation and the
 * copy of tg_csr_builder_append.  Returns 100 like tg_ptap_kron when the kernel declines. */
int tg_ptap_kron_append(tg_csr_t cur, int64_t cur_row0, int d, const int64_t *dims_in,
                        const tg_kron1d_t *fac, int64_t out_row0, int64_t out_row1,
                        const int32_t *zero_dofs, int64_t nzero, double diag, tg_csr_builder_t dest);
/* ---- tensor-pattern extractMatrix (tIGAr/common.py:1176-1204 for tensor-product patches) ----
 * K = M^T A M in three "line walk" passes when A carries the element-coupling pattern of the Q_p node
 * grid (what dolfin assembles for any form on V); the pattern is verified entry by entry while A is read
 * and status 100 means "another pattern: use tg_ptap_kron* / tg_ptap_*".  No column decode, no LDS, no
 * atomics: results are bit-reproducible.  See csrc/tg_tensor_body.h. */
typedef struct {
  int p;                   /* spline degree = degree of the CG Lagrange grid, 1..3                    */
  int nel;                 /* elements; nfe = p*nel+1 FE nodes, ncp = nel+p spline functions           */
  const double *wl;        /* host [nel][p+1][p+1]: value at node p*e+j of spline function e+q         */
} tg_tensor_dir_t;
typedef struct tg_tensor_plan_s *tg_tensor_plan_t;
typedef struct tg_tensor_planes_s *tg_tensor_planes_t;
int tg_tensor_plan_create(int d, const tg_tensor_dir_t *dirs, tg_tensor_plan_t *out);
/* The same plan for ONE BLOCK of a space whose fields sit on different spline bases over one FE node grid -- the
 * components of a div- or curl-conforming B-spline (tIGAr/compatibleSplines.py:21-66: generateFieldsCompat; the spaces of
 * demos/taylor-green/taylor-green-3d.py:42-43), a FieldListSpline (tIGAr/common.py:1949-1970):
 *     K_fg = M_f^T A_fg M_g   with  M_f != M_g.
 * Per direction: p = degree of the FE grid (all fields of such a space extract to one Q_p grid: BSpline.getDegree is the
 * largest directional degree, tIGAr/BSplines.py:580-588), pr / pc = spline degree of the row / column side (<= p), wlr /
 * wlc = their local weights [nel][p+1][p+1] padded with zeros to p + 1 functions per element.  The passes are those of the
 * square plan; the last one writes the true pattern (row function i x column functions [i - pr, i + pc]) and leaves the
 * padding out.  tg_tensor_zstage takes no zero dofs for such a plan (MatZeroRowsColumns acts on the assembled matrix). */
typedef struct {
  int p, nel;
  int pr, pc;
  const double *wlr, *wlc;
} tg_tensor_pair_dir_t;
int tg_tensor_plan_create_pair(int d, const tg_tensor_pair_dir_t *dirs, tg_tensor_plan_t *out);

int tg_tensor_plan_destroy(tg_tensor_plan_t plan);
/* The same for a patch with TWO parametric directions and nfields fields on one scalar basis (M = I (x) M_y (x) M_x,
 * dofs field after field; degrees 1..4): K = M^T A M of the whole matrix in two passes, MatZeroRowsColumns fused.
 * A must hold nfields^2 blocks that all carry the element-coupling pattern (verified; 100 = another pattern). */
int tg_tensor2_plan_create(int nfields, const tg_tensor_dir_t *dirs, tg_tensor_plan_t *out);
/* The same for ONE block (f, g) of fields on different tensor bases over one 2-D Q_P node grid (2-D compatible B-splines,
 * tIGAr/compatibleSplines.py:21-66, demos/taylor-green/taylor-green-2d.py): dirs[2] as for tg_tensor_plan_create_pair;
 * tg_tensor2_ptap then takes the scalar block A_fg and returns K_fg = M_f^T A_fg M_g (no boundary conditions). */
int tg_tensor2_plan_create_pair(const tg_tensor_pair_dir_t *dirs, tg_tensor_plan_t *out);
int tg_tensor2_ptap(tg_tensor_plan_t plan, tg_csr_t a, const int32_t *zero_dofs, int64_t nzero, double diag, tg_csr_t *out);
/* x and y passes over the FE planes [z0,z1) of the last direction; `a` holds FE rows from a_row0 on (whole
 * planes, global columns).  The result (dense blocks, no indices) feeds tg_tensor_zstage and can be kept
 * across sub-slabs. */
int tg_tensor_planes(tg_tensor_plan_t plan, tg_csr_t a, int64_t a_row0, int z0, int z1, tg_tensor_planes_t *out);
int tg_tensor_planes_destroy(tg_tensor_planes_t p);
/* An FE matrix on the plan's node grid with ANOTHER pattern than the element-coupling one (entries added by hand, or
 * missing): on_pattern = the matrix with exactly that pattern holding A's entries that lie on it (zeros elsewhere; it
 * carries the pattern certificate), remainder = the other entries as a CSR matrix of A's shape.
 * M^T A M = M^T on_pattern M (tg_tensor_planes / tg_tensor_zstage) + M^T remainder M (tg_ptap_*), tg_csr_add.
 * Returns 100 when A is not a square matrix on the whole node grid. */
int tg_tensor_split(tg_tensor_plan_t plan, tg_csr_t a, tg_csr_t *on_pattern, tg_csr_t *remainder);
/* z pass: rows of K for the dof planes [ka,kb) from pieces that together hold the FE planes in their support;
 * MatZeroRowsColumns(zero_dofs, diag) fused; appended to `dest` (next rows of a slab-wise builder) or, with
 * dest == NULL, returned as a new matrix in *out. */
int tg_tensor_zstage(tg_tensor_plan_t plan, int npieces, const tg_tensor_planes_t *pieces, int ka, int kb,
                     const int32_t *zero_dofs, int64_t nzero, double diag, tg_csr_builder_t dest, tg_csr_t *out);
/* canonical CSR copy of a loose-row matrix */
int tg_csr_compact(tg_csr_t in, tg_csr_t *out);
int tg_csr_is_loose(tg_csr_t m, int *loose);
int tg_csr_rowptr_at(tg_csr_t m, int64_t r, int64_t *out);   /* rowptr[r], 0 <= r <= nrows */
/* MatZeroRowsColumns(K, zeroDofs, diag) [ext] as called at tIGAr/common.py:1200;
 * K holds global rows [row0, row0+nrows). */
int tg_zero_rows_cols(tg_csr_t k, int64_t row0, const int32_t *dofs, int64_t n, double diag);
/* out = a X + b Y diag(colscale) for X, Y on one sparsity pattern (checked); colscale may be NULL.
 * Tangent matrices J(u) of Newton loops over the path (tIGAr/common.py:1304-1348), e.g.
 * K + M diag(g'(u)): MatAXPY(SAME_NONZERO_PATTERN) + MatDiagonalScale [ext]. */
int tg_csr_combine(double a, tg_csr_t X, double b, tg_csr_t Y, tg_vec_t colscale, tg_csr_t *out);

/* ---- Krylov solve (solveLinearSystem, tIGAr/common.py:1236-1263; seam b-4) -------- */
enum { TG_KSP_CG = 0, TG_KSP_GMRES = 1, TG_KSP_BICGSTAB = 2 };
/* TG_PC_CHEBYSHEV (CG only): `restart` steps of the Chebyshev iteration for D^-1 K on [lmax / ratio, 1.1 lmax] as a fixed
 * polynomial preconditioner (PETSc: PCKSP with KSPCHEBYSHEV + PCJACOBI [ext]; the stand-in for "sor" / "ilu" / "icc" /
 * "bjacobi", which need triangular sweeps); lmax from 20 steps of the power method, capped by the Gershgorin bound. */
enum { TG_PC_NONE = 0, TG_PC_JACOBI = 1, TG_PC_CHEBYSHEV = 2 };
/* status: 0 converged (rtol), 1 converged (atol), -1 max iterations, -2 breakdown/NaN,
 * -3 stagnation (GMRES: 25 restart cycles in a row without progress) */
int tg_krylov_solve(tg_csr_t k, tg_vec_t b, tg_vec_t x, int method, int pc, double rtol,
                    double atol, int maxit, int restart, tg_comm_t comm, int *iters,
                    double *resnorm, int *status);
/* same with flags: TG_KSP_NONZERO_GUESS = x holds the initial guess (dolfin's solver parameter
 * "nonzero_initial_guess" [ext]; the convergence test stays relative to ||B b||, PETSc's default) */
enum { TG_KSP_NONZERO_GUESS = 1, TG_KSP_STAGNATION_GUARD = 2, TG_KSP_SYMMETRIC = 4 };
/* TG_KSP_SYMMETRIC: the caller vouches that k is symmetric (the premise of KSPCG, which PETSc does not check either; set by
 * ExtractedSpline.assembleMatrix for forms that are symmetric by construction): the half-storage copy of a CG solve is still
 * built from rows that are checked one by one against the box stencil, but not compared with the CSR product. */
int tg_krylov_solve_flags(tg_csr_t k, tg_vec_t b, tg_vec_t x, int method, int pc, double rtol,
                          double atol, int maxit, int restart, int flags, tg_comm_t comm, int *iters,
                          double *resnorm, int *status);

/* Fast diagonalization preconditioner for CG on tensor-product patches (csrc/tg_fd.hip): per field block (dofs
 * [offset, offset + prod shape), direction 0 fastest) z = S P^-1 S r on the free box [lo, hi), P the Kronecker sum of the
 * 1-D parametric stiffness / mass matrices with coefficients c_k / c_m, S = D^-1/2 with D = diag K / diag P (or I), and
 * z_i = r_i / K_ii off the box.  tg_fd_add_block takes, per direction k (concatenated over k), the generalized
 * eigenvectors Q_k (nf_k x nf_k, row-major, Q_k^T M_k Q_k = I), their eigenvalues and the diagonals of the 1-D stiffness /
 * mass on the free box (nf_k = hi_k - lo_k <= 4096).  tg_fd_fit records diag K and returns per block the four sums
 * <diag K, t_a> over the free box (rhs[4 b + a]; t_a = diagonal of stiffness term a < d, a = 3 the mass term);
 * tg_fd_set_coefficients takes coef[4 b + a] in the same order (>= 0) and scaling (1 = D^-1/2, 0 = none).
 * tg_fd_apply: z = B r (bit-reproducible).  tg_krylov_solve_fd: CG with it, convergence and status as tg_krylov_solve;
 * flags: TG_KSP_NONZERO_GUESS, TG_KSP_SYMMETRIC. */
int tg_fd_create(int64_t n, tg_fd_t *out);
int tg_fd_add_block(tg_fd_t fd, int d, int64_t offset, const int64_t *shape, const int64_t *lo, const int64_t *hi,
                    const double *Q, const double *lam, const double *dk, const double *dm);
int tg_fd_fit(tg_fd_t fd, tg_csr_t k, double *rhs);
int tg_fd_set_coefficients(tg_fd_t fd, const double *coef, int scaling);
int tg_fd_apply(tg_fd_t fd, tg_vec_t r, tg_vec_t z);
int tg_fd_destroy(tg_fd_t fd);
int tg_krylov_solve_fd(tg_csr_t k, tg_fd_t fd, tg_vec_t b, tg_vec_t x, double rtol, double atol, int maxit, int flags,
                       int *iters, double *resnorm, int *status);

/* Block kernels of the LOBPCG eigensolver (csrc/tg_eig.hip; tigar_amd/eigen.py).  A block is a tg_vec_t of n * k doubles,
 * row-major (entry (i, j) at i * k + j), 1 <= k <= 64 (other widths: error).  Every result is bit-reproducible (fixed
 * summation orders, no floating-point atomics).  tg_spmm: Y = A X for a canonical CSR A (loose-row / view CSRs: error), A
 * read once.  tg_block_gram: G = X^T Y (kx x ky, row-major, host).  tg_block_combine: Y = sum_s X_s C_s over the inputs
 * that are not null (C_s: k_s x ky, row-major, host; Y must not be an input).  tg_block_residual: R = AX - BX diag(lam)
 * with the rows where mask != 0 zeroed, W = dinv .* R (W = R without dinv; W optional), rnorm2[j] = |R_j|^2 and
 * bxnorm2[j] = |BX_j|^2 (optional) on the host.  tg_block_get_column / tg_block_set_column: column j of X to / from v.
 * tg_csr_decoupled_rows: mark[i] = 1 where the only non-zero of row i of A and of B (B null = identity) is the diagonal,
 * 0 elsewhere, da / db = the diagonals, *count = rows marked, *arow (optional) = the largest sum of |a_ij| over the rows
 * not marked.  tg_csr_sym_defect: max |A - at| over the union pattern and
 * max |A_ij| over i != j (the scale: a penalty on the diagonal does not hide a defect) for at = tg_csr_transpose(A) (rows of both ascending; *unsorted = 1 when a row of A is not). */
int tg_spmm(tg_csr_t a, tg_vec_t x, int k, tg_vec_t y);
int tg_block_gram(tg_vec_t x, int kx, tg_vec_t y, int ky, int64_t n, double *g_host);
int tg_block_combine(tg_vec_t y, int ky, int64_t n, tg_vec_t x0, int k0, const double *c0, tg_vec_t x1, int k1,
                     const double *c1, tg_vec_t x2, int k2, const double *c2);
int tg_block_residual(tg_vec_t ax, tg_vec_t bx, const double *lam, int k, int64_t n, tg_vec_t mask, tg_vec_t dinv,
                      tg_vec_t r, tg_vec_t w, double *rnorm2, double *bxnorm2);
int tg_block_get_column(tg_vec_t x, int k, int j, tg_vec_t v);
int tg_block_set_column(tg_vec_t x, int k, int j, tg_vec_t v);
int tg_csr_decoupled_rows(tg_csr_t a, tg_csr_t b, tg_vec_t mark, tg_vec_t da, tg_vec_t db, int64_t *count,
                          double *arow);
int tg_csr_sym_defect(tg_csr_t a, tg_csr_t at, double *defect, double *amax, int *unsorted);

/* generateM for a spline given by element-wise Bezier extraction operators (Rhino T-splines,
 * tIGAr/RhinoTSplines.py:37-137 + the row loop of tIGAr/common.py:1554-1571): FE row (e, n) holds
 * N_a = sum_b coef[a][b] * bern[e][n][b] for the functions a of element e (eoff[e] <= a < eoff[e+1], global index
 * nodes[a] + col_offset, ascending per element), entries with abs(v) <= eps dropped. */
int tg_extract_csr_bezier(int64_t nel, int nloc, int nbern, const double *bern, const int64_t *eoff,
                          const int32_t *nodes, const double *coef, int32_t col_offset, int64_t ncols, double eps,
                          tg_csr_t *out);

/* ---- direct solve: what solveLinearSystem runs when linearSolver is None (dolfin solve() = sparse LU [ext],
 * tIGAr/common.py:1255-1256).  Banded LU with partial pivoting in LAPACK's dgbtrf storage / pivoting scheme. */
/* half-bandwidths of a square matrix and the bytes its band storage (2*kl+ku+1 rows) would take */
int tg_lu_band_info(tg_csr_t k, int *kl, int *ku, int64_t *bytes);
/* x = K^-1 b (x may be b); info > 0: U(info-1,info-1) == 0 exactly, nothing was solved */
int tg_lu_solve(tg_csr_t k, tg_vec_t b, tg_vec_t x, int *info);
/* The same system by a blocked banded Cholesky factorisation on the matrix cores (csrc/tg_chol.hip) when K is symmetric
 * (values compared with their transposes) and positive definite (every pivot positive): *done = 1 and x = K^-1 b (x may
 * be b); otherwise *done = 0 and x is untouched.  tg_lu_solve tries this itself first; the entry exists for systems
 * beyond the LU's limits (3-D patches: n kl^2 multiply-adds and n (kl + 1) doubles instead of 4 n kl^2 and 3 n kl), where
 * the caller's alternative is a Krylov method (tigar_amd.common._DefaultSolver). */
int tg_chol_solve(tg_csr_t k, tg_vec_t b, tg_vec_t x, int *done);

/* ---- synthetic FE-side input (NOT on the timed path) --------- */
/* A = sum_t (x)_k F[t][k] with 1-D CSR factors sharing one pattern per direction
 * (e.g. Q_p Laplace stiffness = K1xM1xM1 + M1xK1xM1 + M1xM1xK1); rows [row0,row1). */
typedef struct {
  int64_t n;               /* 1-D size                                   */
  const int32_t *rowptr;   /* n+1                                        */
  const int32_t *col;      /* shared pattern                             */
  const double *val;       /* nterms * nnz1d values, term-major          */
} tg_kron_dir_t;
int tg_kron_sum_csr(int d, int nterms, const tg_kron_dir_t *dirs, int64_t row0,
                    int64_t row1, tg_csr_t *out);
/* The same planes for an FE matrix GIVEN AS A KRONECKER SUM of 1-D matrices (dirs[k]: the 1-D pattern of direction k
 * and nterms value sets, term-major -- the arguments of tg_kron_sum_csr): the matrix is never written, its entries are
 * formed inside the x pass exactly as tg_kron_sum_csr forms them, so the planes are bit for bit those of
 * tg_tensor_planes on the materialised matrix.  100: the 1-D patterns are not the element-coupling patterns of the
 * plan, or more than three terms (materialise and call tg_tensor_planes).  SURVEY 8(d): "If the build fuses A-generation
 * into PtAP (never materialising A) ...". */
int tg_tensor_planes_kron(tg_tensor_plan_t plan, int nterms, const tg_kron_dir_t *dirs, int z0, int z1,
                          tg_tensor_planes_t *out);
/* FE planes that `p` holds, and how many of them the x and y passes contracted.  tg_tensor_planes_kron contracts one
 * plane per class of planes whose rows of dirs[2] are equal bit for bit in every term (their blocks are equal bit for
 * bit; the others share them) unless TIGAR_TT_PLANE_CLASSES=0; tg_tensor_planes contracts every plane. */
int tg_tensor_planes_info(tg_tensor_planes_t p, int *n_planes, int *n_contracted);
/* The last tg_tensor_zstage of `plan`: the FE planes it walked, the B2 blocks a lane loaded on the way, and whether the
 * walk held the last block of every node slot of an element in registers.  It does when some plane has the block of the
 * plane p before it (planes sharing blocks, above) unless TIGAR_TT_Z_CACHE=0, and then loads one block per change of
 * pointer in a slot; the plain walk loads one per plane.  K is the same bit for bit. */
int tg_tensor_zstage_info(tg_tensor_plan_t plan, int *held, int *n_planes, int *n_block_loads);

/* General Kronecker-product CSR builder on the device: out = sum_t (x)_k F[t][k] restricted to rows
 * [row0,row1), with rectangular 1-D factors (cdim[k] = number of columns of direction k; NULL =
 * square), optional |v| > eps filter (single term), a column offset and a total column count
 * (-1 = prod cdim).  Used for the directional extraction operators I(x)I(x)M_x ... of the
 * sum-factorised M^T A M and for their transposes. */
int tg_kron_csr_rect(int d, int nterms, const tg_kron_dir_t *dirs, const int64_t *cdim, int64_t row0,
                     int64_t row1, int filter, double eps, int64_t col_offset, int64_t ncols_total,
                     tg_csr_t *out);
/* generateM / its transpose for a tensor-product B-spline whose abs(v) > eps filter drops nothing but exact zeros
 * (the caller checks that on the 1-D tables): out = F[2] (x) F[1] (x) F[0] restricted to rows [row0,row1), values
 * (v0*v1)*v2 in the reference's order (tIGAr/BSplines.py:450-503), written by a pencil walk with closed-form row
 * starts (no count pass, no scan); cdim[k] = columns of direction k; columns shifted by col_offset. */
int tg_kron3_csr(int d, const tg_kron_dir_t *dirs, const int64_t *cdim, int64_t row0, int64_t row1,
                 int64_t col_offset, int64_t ncols_total, tg_csr_t *out);

/* One 1-D sparse factor F (nout_k rows, CSR on the host, columns in [col_shift, col_shift+dims_in[k]))
 * applied along direction k of a tensor-indexed vector (direction 0 fastest):
 *     out[lo, I, hi] = sum_t F[I, c_t] in[lo, c_t - col_shift, hi].
 * Three such passes give M^T b (multTranspose, tIGAr/common.py:97-109) and M U (:1259) of a
 * Kronecker-structured extraction operator without forming M or M^T. */
int tg_tensor_apply_1d(int d, const int64_t *dims_in, int k, int64_t nout_k, const int32_t *rowptr,
                       const int32_t *col, const double *val, int64_t col_shift, tg_vec_t in, tg_vec_t out);

/* ---- FE-side operator assembly on mapped tensor-product patches ----
 * Stands in for dolfin.assemble(form) (tIGAr/common.py:1206-1220) with the spline's measures:
 * geometry F = cp[i]/cp[nsd] (tIGAr/common.py:917-921), metric g = DF^T DF, volume element
 * sqrt(det g) (tIGAr/calculusUtils.py:66-70), Cartesian gradient through pinv(DF)
 * (tIGAr/calculusUtils.py:56-64), Gauss-Legendre quadrature with nq points per direction
 * (quadrature_degree 2p <-> nq = p+1).  Scalar Q_p Lagrange space on the tensor node grid with
 * direction 0 fastest; nsd >= d (surfaces: Laplace-Beltrami). */
typedef struct {
  int d, p;                 /* parametric dimension, FE degree                        */
  const double *verts[3];   /* element vertices per direction (host), nverts[k] each  */
  int nverts[3];
  int nsd;                  /* physical dimension, d <= nsd <= 3                      */
  tg_vec_t cp[4];           /* nsd+1 homogeneous control functions on the FE nodes    */
  int nq;                   /* Gauss points per direction                             */
} tg_patch_t;
/* limits of the element kernels on these patches: (p+1)^d local nodes, Gauss points per direction (no device needed) */
int tg_assemble_limits(int *max_local_nodes, int *max_gauss_points);
/* form: 0 = (u,v), 1 = (grad u, grad v), 4 = (lap u, lap v) element by element with lap = spline.div(spline.grad(.)) and
 * the second derivatives of the map (nsd == d; demos/biharmonic/biharmonic.py:100-103); result on the element-coupling
 * pattern */
int tg_assemble_mapped_matrix(const tg_patch_t *patch, int form, tg_csr_t *out);
/* L(v) = (f_h, v) with f_h the nodal interpolant of fnodal */
int tg_assemble_mapped_load(const tg_patch_t *patch, tg_vec_t fnodal, tg_vec_t out);
/* Row blocks of the same objects, as the z-slab pipeline of extractMatrix / extractVector consumes them (PETSc's row-block
 * MatPtAP, tIGAr/common.py:1194-1195; the assembled matrix of BASELINE cfg3 would hold 684 GB): rows [row0, row1) = whole
 * node planes of the LAST direction, global column indices, the element-coupling pattern with its certificate
 * (tg_tensor_planes then reads no column index).  patch->cp[c] (and fnodal) hold the FE nodes [cp_node0, cp_node0 + n) --
 * a window that must cover every element touching the rows -- so a rank never needs the control functions outside its
 * slab.  3-D patches with nq = p + 1 <= 4: sum-factorised element matrices, one wave per element
 * (csrc/tg_assemble.hip, k_asf3). */
int tg_assemble_mapped_matrix_rows(const tg_patch_t *patch, int form, int64_t row0, int64_t row1, int64_t cp_node0,
                                   tg_csr_t *out);
int tg_assemble_mapped_load_rows(const tg_patch_t *patch, tg_vec_t fnodal, int64_t row0, int64_t row1, int64_t cp_node0,
                                 tg_vec_t out);
/* Block (fi, fj) of linear elasticity a(u,v) = int lambda div u div v + 2 mu eps(u):eps(v) dx on the mapped patch, u, v in
 * the d-field space on the patch's node grid (nsd == d): lambda (d_fi phi_a, d_fj phi_b) + mu (d_fj phi_a, d_fi phi_b)
 * + delta mu (grad phi_a, grad phi_b) with the Cartesian derivatives of spline.grad / spline.div (tIGAr/common.py:1022-1040,
 * calculusUtils.py:255-276) -- what dolfin.assemble gives for inner(sigma(u), eps(v))*spline.dx restricted to test
 * component fi, trial component fj.  Rows and control-function window as tg_assemble_mapped_matrix_rows
 * (row0 = row1 = -1: the whole block); same pattern, same kernels (the coefficient tensor per point is not symmetric). */
int tg_assemble_mapped_elasticity_rows(const tg_patch_t *patch, int fi, int fj, double lambda, double mu, int64_t row0,
                                       int64_t row1, int64_t cp_node0, tg_csr_t *out);

/* ---- quadrature-point evaluation on the same patches (csrc/tg_postproc.hip): L2 projection (tIGAr/common.py:1392-1433)
 * and error norms (the demos' sqrt(assemble(((u-soln)**2)*spline.dx))) need the points, u_h and its Cartesian gradient
 * there, a load vector from point values and three weighted sums.  Points are numbered element-major: elements
 * lexicographic with direction 0 fastest, the nq^d Gauss points of an element likewise; npts = nq^d prod nel_k.  Arrays
 * with nsd components per point are component-major (component c of point q at c npts + q).  The control functions are
 * given on all FE nodes.  Sum-factorised, no floating-point atomics: the same inputs give the same bits. */
/* x_q = F(xi_q) = cp[i]/cp[nsd] (nsd npts values) and wdet_q = w_q sqrt(det g) prod h_k, the weight of every form above */
int tg_quad_points(const tg_patch_t *patch, tg_vec_t x_out, tg_vec_t wdet_out);
/* u_h(x_q) of a nodal vector; with_grad: also the Cartesian gradient DF g^-1 grad_xi u_h (pinv(DF) and the quotient rule
 * of the rational map, the operator of form 1) into grad_out (nsd npts values; ignored without with_grad) */
int tg_quad_eval(const tg_patch_t *patch, tg_vec_t u_nodal, int with_grad, tg_vec_t val_out, tg_vec_t grad_out);
/* out[node] = sum_q wdet_q f_q phi_node(xi_q): the load vector of a function given by its values at the points */
int tg_quad_load(const tg_patch_t *patch, tg_vec_t f_q, tg_vec_t out);
/* out[0] = sum wdet (u_h - e)^2, out[1] = sum wdet |grad u_h - ge|^2, out[2] = sum wdet e^2 (host array of 3).  e_q (npts)
 * and ge_q (nsd npts) may be null: the term is 0; u_nodal may be null: u_h = 0 */
int tg_quad_error(const tg_patch_t *patch, tg_vec_t u_nodal, tg_vec_t e_q, tg_vec_t ge_q, double *out);

/* ---- rational (NURBS) trial and test functions ----------------------------------------------------------------------
 * The reference's demos solve in the rational space: u = spline.rationalize(TrialFunction(V)), v likewise
 * (demos/poisson/poisson-nurbs.py:121-124; ExtractedSpline.project, tIGAr/common.py:1408-1409), i.e. with the basis
 * psi_a = phi_a / W_h, W_h = cp[nsd] interpolated.  With beta = grad_xi W_h / W_h, grad_xi psi_a = (grad_xi phi_a -
 * phi_a beta) / W_h: every point coefficient of the entries above carries over -- the tensor of the stiffness / elasticity
 * integrand acts on (grad_xi phi - phi beta) with the factor 1 / W_h^2, the mass weight takes 1 / W_h^2, the load 1 / W_h
 * (f_h stays the nodal interpolant of fnodal).  Same pattern, same symmetry, same arguments and row blocks as the twins
 * without `rational` (row0 = row1 = -1: all rows); the same bits for the same inputs.  With unit weights the results are
 * those of the twins up to rounding.  3-D, nq = p + 1, p = 2, 3: mass, stiffness and load run sum-factorised; p = 1 and
 * the elasticity blocks take the plain element kernel, for every shape it takes for the twins (the rational stiffness /
 * elasticity of a shape whose twin fills the 64 KiB of LDS a launch gets by itself asks for up to 13 KB more).
 * form: 0 = mass, 1 = laplace (no rational biharmonic form). */
int tg_assemble_rational_matrix_rows(const tg_patch_t *patch, int form, int64_t row0, int64_t row1, int64_t cp_node0,
                                     tg_csr_t *out);
int tg_assemble_rational_elasticity_rows(const tg_patch_t *patch, int fi, int fj, double lambda, double mu, int64_t row0,
                                         int64_t row1, int64_t cp_node0, tg_csr_t *out);
int tg_assemble_rational_load_rows(const tg_patch_t *patch, tg_vec_t fnodal, int64_t row0, int64_t row1, int64_t cp_node0,
                                   tg_vec_t out);
/* u = u_h / W_h at the points and its Cartesian gradient DF g^-1 (grad_xi u_h - u grad_xi W_h) / W_h */
int tg_quad_eval_rational(const tg_patch_t *patch, tg_vec_t u_nodal, int with_grad, tg_vec_t val_out, tg_vec_t grad_out);
/* out[node] = sum_q wdet_q f_q phi_node(xi_q) / W_h(xi_q) */
int tg_quad_load_rational(const tg_patch_t *patch, tg_vec_t f_q, tg_vec_t out);
/* the three sums of tg_quad_error with u = u_h / W_h */
int tg_quad_error_rational(const tg_patch_t *patch, tg_vec_t u_nodal, tg_vec_t e_q, tg_vec_t ge_q, double *out);

/* ---- volume forms with point coefficients (csrc/tg_coef.hip, endings of csrc/tg_postproc.hip) ------------------------------
 *   a(u, v) = int grad v . (A grad u) + (b . grad v) u + v (c . grad u) + m u v dx     (u: trial = column, v: test = row)
 *   L(v)    = int s v + F . grad v dx
 * on the patches above (scalar Q_p space, d = 1, 2, 3, nsd >= d), grad the Cartesian gradient DF g^-1 grad_xi, with A, b, c,
 * m, s, F given at the quadrature points, numbered as tg_quad_points, vectors and tensors component-major (component (i, j)
 * of A at (i nsd + j) npts + q).  Any point array may be null: zero.
 * tg_coef_transform: one pass over the points, Cartesian data -> reference element.  With P = DF g^-1 and wdet = w sqrt(det g):
 * C^ = wdet P^T A P, b^ = wdet P^T b, c^ = wdet P^T c, m^ = wdet m -- coef_out holds (d^2 + 2 d + 1) npts values,
 * component-major: C^ row-major (d^2), b^ (d), c^ (d), m^.  a_kind: 0 no diffusion (A_q null), 1 one value per point
 * (A = a I), 2 an nsd x nsd tensor per point, which need not be symmetric.  rational != 0: trial and test functions
 * phi / W_h; with beta = grad_xi W_h / W_h the data become C' = C^ / W^2, b' = b^ / W^2 - C' beta, c' = c^ / W^2 - C'^T beta,
 * m' = m^ / W^2 - beta . b^ / W^2 - beta . c^ / W^2 + beta . C' beta, so that the matrix entry needs no rational twin.
 * tg_flux_transform: s^ = wdet s, F^ = wdet P^T F ((d + 1) npts values: s^, then F^); rational: F' = F^ / W,
 * s' = (s^ - F^ . beta) / W. */
int tg_coef_transform(const tg_patch_t *patch, int rational, int a_kind, tg_vec_t A_q, tg_vec_t b_q, tg_vec_t c_q, tg_vec_t m_q,
                      tg_vec_t coef_out);
int tg_flux_transform(const tg_patch_t *patch, int rational, tg_vec_t s_q, tg_vec_t F_q, tg_vec_t out);
/* A_ab = sum_q grad_xi phi_a . C_q grad_xi phi_b + (b_q . grad_xi phi_a) phi_b + phi_a (c_q . grad_xi phi_b) + m_q phi_a phi_b
 * from the output of tg_coef_transform, on the element-coupling pattern with its certificate (the pattern of every mapped
 * form).  All rows; colours in the order of the other element kernels, no floating-point atomics, the same bits in every run.
 * 3-D, nsd = 3, nq = p + 1, p = 2, 3: sum-factorised instantiations of k_asf3 (p = 2, the walk) and k_asf3_quad (p = 3) whose
 * phase 0 loads the point data (csrc/tg_assemble.hip); TIGAR_ASM_LEGACY selects the plain kernel (csrc/tg_coef.hip), which
 * takes every other shape; TIGAR_ASM_CHUNK / TIGAR_ASM_QUAD_CHUNK size the pieces as for the stiffness matrix.
 * The patch gives the shape (d, p, nq, element counts); its control functions are not read, and its element vertices serve
 * the cache of the reference-element tables only.  Nothing ties `coef` to the patch, nq or rational setting it was
 * transformed for but its length: a mismatch of nq between transform and assembly is caught only when the sizes differ. */
int tg_assemble_coef_matrix(const tg_patch_t *patch, tg_vec_t coef, tg_csr_t *out);
/* ---- vector-valued unknowns with a point tangent: nF = nsd = d (2 or 3) fields on the scalar Q_p space, dofs field after
 * field (the space of the mapped elasticity form), a(u, v) = int d_K v_i A_iKjL d_L u_j + v_i M_ij u_j dx.
 * tg_coef_transform_blocks: A_q holds A_iKjL at (((i nF + j) nsd + K) nsd + L) npts + q -- block (i, j) a contiguous nsd x nsd
 * tensor in the layout of a_kind = 2 --, M_q (may be null) M_ij at (i nF + j) npts + q.  coef_out: nF^2 consecutive scalar
 * coefficient sets of (d^2 + 2 d + 1) npts values each, block (i, j) at (i nF + j), every one in the layout of
 * tg_coef_transform (rational: b', c', m' per block as there).  One pass: the geometry of a point is formed once for all
 * blocks (an ending of k_postproc).
 * tg_assemble_coef_blocks: every block through tg_assemble_coef_matrix on a view of its slice (same routes and environment
 * variables), then tg_csr_from_blocks: the nF n x nF n matrix, rows and columns field-major.
 * Point data held at the peak of one tangent assembly: A_q (d^4 npts) and the transformed sets (d^2 (d^2 + 2 d + 1) npts),
 * i.e. (d^4 + 16 d^2) npts = 225 npts doubles at d = 3 (52 npts at d = 2). */
int tg_coef_transform_blocks(const tg_patch_t *patch, int rational, int nF, tg_vec_t A_q, tg_vec_t M_q, tg_vec_t coef_out);
int tg_assemble_coef_blocks(const tg_patch_t *patch, int nF, tg_vec_t coef_blocks, tg_csr_t *out);
/* ---- first-order systems: nF >= 1 fields (at most 16) on the scalar Q_p space, dofs field after field, d = 1, 2, 3, nsd >= d,
 * nF independent of nsd:
 *   a(u, v) = sum_ij int d_K v_i A_iKjL d_L u_j + d_K v_i b_iKj u_j + v_i c_ijL d_L u_j + v_i m_ij u_j dx
 * tg_coef_transform_system: block (i, j) = test field i, trial field j, each with its own data -- A_q holds A_iKjL at
 * (((i nF + j) nsd + K) nsd + L) npts + q, b_q holds b_iKj at ((i nF + j) nsd + K) npts + q, c_q holds c_ijL at
 * ((i nF + j) nsd + L) npts + q, M_q holds m_ij at (i nF + j) npts + q; any of the four may be null: zero.  coef_out: the layout
 * of tg_coef_transform_blocks (nF^2 sets of (d^2 + 2 d + 1) npts values).  The same ending of k_postproc with the same
 * per-block body: with b_q and c_q null the bits of tg_coef_transform_blocks, with nF = 1 those of tg_coef_transform(a_kind =
 * 2) (a_kind = 0 where A_q is null).
 * tg_assemble_coef_system: tg_assemble_coef_blocks for such a set of blocks, any nF (nF = 1: the block itself).
 * tg_quad_metric: the element metric G = 4 P P^T, P = DF g^-1 -- d xi / d x of the BI-UNIT parent element contracted over
 * the parametric index, the G of the stabilisation parameters of tg_flow_points; nsd^2 npts values, symmetric, all
 * components stored, G_KL at (K nsd + L) npts + q; nsd >= d (rank d). */
int tg_coef_transform_system(const tg_patch_t *patch, int rational, int nF, tg_vec_t A_q, tg_vec_t b_q, tg_vec_t c_q, tg_vec_t M_q,
                             tg_vec_t coef_out);
int tg_assemble_coef_system(const tg_patch_t *patch, int nF, tg_vec_t coef_blocks, tg_csr_t *out);
int tg_quad_metric(const tg_patch_t *patch, tg_vec_t G_out);
/* ---- the incompressible Navier-Stokes law at the points (csrc/tg_flow.hip): nsd = 2, 3, nF = nsd + 1 fields (u, p), Galerkin +
 * SUPG + PSPG + LSIC.  params = {rho, mu, c_a, 4 / dt^2, C_I} (host), nu = mu / rho; a = c_a u + a0.
 *   r_i = rho (a_i + u_L d_L u_i - f_i) + d_i p (the viscous part is left out), tau_M = (4 / dt^2 + u . G u + C_I nu^2 G:G)^(-1/2),
 *   tau_C = 1 / (tau_M tr G);  s_i = r_i - d_i p,  F_iK = mu (d_K u_i + d_i u_K) - p d_iK + tau_M u_K r_i + rho tau_C div u d_iK,
 *   s_p = div u,  F_pK = (tau_M / rho) r_K.
 * U_q: field i at i npts + q; gradU_q: d U_i / d x_K at (i nsd + K) npts + q; a0_q, f_q (may be null: zero): nsd npts values;
 * G_q: tg_quad_metric.  s_out (nF npts) and F_out (nF nsd npts) in the layout of tg_quad_load_flux per field; A_out, b_out,
 * c_out, M_out: the exact derivative of (s, F), tau included, in the layouts of tg_coef_transform_system, dense (zeros
 * written); tau_out: tau_M (npts), then tau_C (npts).  Any output may be null; every subset gives the same bits.  No atomics. */
int tg_flow_points(const double *params, int nsd, int64_t npts, tg_vec_t U_q, tg_vec_t gradU_q, tg_vec_t a0_q, tg_vec_t f_q,
                   tg_vec_t G_q, tg_vec_t s_out, tg_vec_t F_out, tg_vec_t A_out, tg_vec_t b_out, tg_vec_t c_out, tg_vec_t M_out,
                   tg_vec_t tau_out);
/* ---- evaluation at points the caller chooses, closest points (csrc/tg_sample.hip) --------------------------------------------
 * The patches of the point kernels above: d = 1, 2, 3, nsd >= d, (p+1)^d <= the limit of tg_assemble_limits, control functions
 * on all FE nodes; patch->nq is not read.  Point arrays are component-major (component c of point q at c npts + q); npts is
 * taken from the length of the input vector; npts = 0: no launch, status 0.  One lane per point, grids capped at 1024 workgroups
 * of 256 lanes (p <= 4: 1-D tables in registers) or 64 lanes (p > 4: tables in LDS) that stride over the rest; no atomics: a
 * point's result depends on that point alone, the same inputs give the same bits.
 * LOCATION RULE: a point is inside iff v_k[0] <= xi_k <= v_k[last] for every k, by exact comparisons; its element in
 * direction k is the largest e <= nel_k - 1 with v_k[e] <= xi_k (a point on an interior vertex belongs to the upper element,
 * the last vertex to the last element); the local coordinate is t = (xi_k - v_k[e]) / (v_k[e+1] - v_k[e]).
 * tg_point_eval: xi holds d npts parametric (knot) coordinates; u_nodal nF >= 1 fields on the grid, field after field (null:
 *   only x_out).  Any output may be null: x_out (nsd npts) = F(xi) = cp[i]/cp[nsd]; val_out (nF npts), field i at i npts + q;
 *   grad_out (nF nsd npts), the Cartesian gradient DF g^-1 grad_xi, component K of field i at (i nsd + K) npts + q (the layout
 *   of tg_flow_points).  rational: u_h / W_h and its gradient by the quotient rule, as tg_quad_eval_rational.  A point that
 *   is not inside (NaN and +-inf included) gets NaN in every output and no field is read for it.
 * tg_point_locate: the closest point of the patch to each of the npts physical points x (nsd npts values): the minimiser of
 *   |x - F(xi)|^2 over the parametric box -- the inverse map for nsd = d and x in the image, the projection otherwise.
 *   1. Seed: the point's entry of xi_guess (d npts values, clipped to the box) if given; else the nearest centre F(xi_c) among
 *      the elements of a sub-lattice: every s_k-th element of direction k (elements 0, s_k, 2 s_k, ...), the strides grown from
 *      (1, 1, 1) -- the direction with the most seeds first, the lowest on a tie -- until at most max_seeds seeds are left;
 *      brute force, ties to the lowest seed index (direction 0 fastest).
 *   2. Step: Gauss-Newton, delta = (DF^T DF)^-1 DF^T r, r = x - F(xi), formed in coordinates scaled by the box (range_k).  A
 *      direction whose bound is active and whose gradient component (DF^T r)_k points outward is held.  The scaled normal
 *      matrix counts as singular when its determinant is not above 1e-20 (largest diagonal entry)^d: status 3.
 *   3. Update: xi + delta clipped to the box; the step is halved (at most 10 times) while |r|^2 does not decrease, where a
 *      change below sum_c e_c (2 |r_c| + e_c), e_c = 32 eps (|x_c| + |F_c|), counts as rounding and not as an increase.  No
 *      decrease after the last halving: status 1.
 *   4. Stop when max_k |clip(xi + delta)_k - xi_k| / range_k <= tol (that last full step is taken): status 0; or after max_iter
 *      (1..100) steps: status 1.
 *   xi_out (d npts) always lies inside the box.  info_out (3 npts): the distance |x - F(xi)| at q, the number of steps at
 *   npts + q, the status at 2 npts + q: 0 converged, 1 iteration limit, 2 input not finite (xi = NaN, distance NaN),
 *   3 singular DF^T DF.  No second derivatives enter: for a non-zero residual the convergence is LINEAR with the ratio
 *   ~ distance x curvature (no convergence beyond the centre of curvature). */
int tg_point_eval(const tg_patch_t *patch, int nF, tg_vec_t u_nodal, tg_vec_t xi, int rational, tg_vec_t x_out, tg_vec_t val_out,
                  tg_vec_t grad_out);
int tg_point_locate(const tg_patch_t *patch, tg_vec_t x, tg_vec_t xi_guess, double tol, int max_iter, int64_t max_seeds,
                    tg_vec_t xi_out, tg_vec_t info_out);
/* ---- sampling on a lattice (endings 0 and 1 of csrc/tg_postproc.hip): m caller-given abscissae t[0..m) (host, increasing, in
 * [0, 1], the ends allowed) per element and direction, 1 <= m <= the Gauss-point limit.  Numbering and layouts of
 * tg_quad_points / tg_quad_eval with m for nq (points on shared element faces come once per element). */
int tg_lattice_points(const tg_patch_t *patch, int m, const double *t, tg_vec_t x_out);
int tg_lattice_eval(const tg_patch_t *patch, int m, const double *t, tg_vec_t u_nodal, int with_grad, tg_vec_t val_out,
                    tg_vec_t grad_out);
int tg_lattice_eval_rational(const tg_patch_t *patch, int m, const double *t, tg_vec_t u_nodal, int with_grad, tg_vec_t val_out,
                             tg_vec_t grad_out);
/* ---- material laws at the points (csrc/tg_material.hip): F = I + grad u, J = det F, C = F^T F, nsd = 2 (plane strain) or 3.
 * gradu: d u_i / d x_K at (i nsd + K) npts + q; P_out: the first Piola-Kirchhoff stress in the same layout; A_out:
 * A_iKjL = d P_iK / d F_jL in the layout of tg_coef_transform_blocks; psi_out: the energy density; any output may be null.
 * params = {lambda, mu} (host).  kind 0 linear: psi = lambda/2 (tr eps)^2 + mu eps:eps; 1 St. Venant-Kirchhoff:
 * S = lambda tr E I + 2 mu E, P = F S; 2 compressible neo-Hookean: psi = mu/2 (tr C - nsd) - mu ln J + lambda/2 (ln J)^2.
 * Kind 2 writes nothing at a point with J <= 0; *nbad counts those points, *Jmin is the smallest J of all points (any kind;
 * kinds 0 and 1 count no point).  Integer atomics only: the same bits in every run.  Synchronises the stream. */
int tg_material_points(int kind, const double *params, int nsd, int64_t npts, tg_vec_t gradu, tg_vec_t P_out, tg_vec_t A_out,
                       tg_vec_t psi_out, int64_t *nbad, double *Jmin);
/* out[node] = sum_q wdet_q (s_q phi_node + F_q . grad phi_node)(xi_q), the Cartesian gradient; either array may be null.
 * _rational: tested against phi / W_h.  Sum-factorised both ways, added colour by colour as tg_quad_load. */
int tg_quad_load_flux(const tg_patch_t *patch, tg_vec_t s_q, tg_vec_t F_q, tg_vec_t out);
int tg_quad_load_flux_rational(const tg_patch_t *patch, tg_vec_t s_q, tg_vec_t F_q, tg_vec_t out);
/* ---- second-derivative point forms (csrc/tg_jet.hip): d = 1, 2, nsd >= d, the scalar Q_p space; nF >= 1 fields share it,
 * dofs field after field.  The JET of a function at a point: value | first | second derivatives (order 00, 01, 11) with
 * respect to the patch's parametric (knot) coordinates xi -- spline.parametricGrad of the reference --, nJ = 3 (d = 1) or 6
 * (d = 2) components; component alpha of field i at (i nJ + alpha) npts + q, points numbered as tg_quad_points.
 * With S = diag(1, 1/h_k, 1/(h_k h_m)) (h: the element's sizes) and L the lower-triangular matrix of the quotient rule
 * jet(phi / W_h) = L jet(phi) (identity without `rational`), Q = S L_ref:  jet_xi(u) = Q jet_ref(u_h).
 * tg_quad_jet: nJ npts values of u_h (rational: u_h / W_h).  tg_quad_geometry_jet: nsd nJ npts values of x = N / W,
 *   component c at (c nJ + alpha) npts + q.
 * tg_jet_transform: nblk blocks of nJ x nJ point matrices T (row alpha: test, column beta: trial) at
 *   (b nJ^2 + alpha nJ + beta) npts + q  ->  T' = wdet Q^T T Q in the same layout (wdet: the weight of tg_quad_points); the
 *   point's geometry, W-jet and Q are formed once for all blocks.  tg_jet_load_transform: s' = wdet Q^T s for nF fields.
 *   Input and output must be different vectors.
 * tg_assemble_jet_blocks: block (i, j), A_e[a][b] = sum_q sum_{alpha beta} J^alpha_ref phi_a T'^{alpha beta}_{ij,q} J^beta_ref phi_b,
 *   each on the element-coupling pattern with its certificate, put together by tg_csr_from_blocks (nF = 1: the block
 *   itself); any nF >= 1.  `coef`: nF^2 consecutive sets of tg_jet_transform.  The control functions of the patch are not read.
 * tg_quad_load_jet: out[i n + a] = sum_q sum_alpha s'^alpha_{i,q} J^alpha_ref phi_a, an output of nF n values, zeroed here.
 * The matrix and the load add colour by colour without floating-point atomics: the same inputs give the same bits. */
int tg_quad_jet(const tg_patch_t *patch, tg_vec_t u_nodal, int rational, tg_vec_t jet_out);
int tg_quad_geometry_jet(const tg_patch_t *patch, tg_vec_t jet_out);
int tg_jet_transform(const tg_patch_t *patch, int rational, int nblk, tg_vec_t T_q, tg_vec_t coef_out);
int tg_jet_load_transform(const tg_patch_t *patch, int rational, int nF, tg_vec_t s_q, tg_vec_t out);
int tg_assemble_jet_blocks(const tg_patch_t *patch, int nF, tg_vec_t coef, tg_csr_t *out);
int tg_quad_load_jet(const tg_patch_t *patch, int nF, tg_vec_t s_t, tg_vec_t out);
/* ---- Kirchhoff-Love shell laws at the points (csrc/tg_shell.hip): d = 2, nsd = nF = 3.  Xjet: the jets of the reference
 * surface (tg_quad_geometry_jet), ujet: those of the three displacement fields (tg_quad_jet per field, one after the other),
 * 18 npts values each, component alpha of coordinate / field c at (6 c + alpha) npts + q; x = X + u.
 * kind 0, params = {E, nu, thickness} (host): psi = h/2 eps:C:eps + h^3/24 kappa:C:kappa per unit reference area, with
 * eps_ab = (a_ab - A_ab)/2, kappa_ab = B_ab - b_ab, C^abcd = E/(1 - nu^2) [nu A^ab A^cd + (1 - nu)/2 (A^ac A^bd + A^ad A^bc)].
 * psi_out: npts values; s_out = d psi / d jet(u): 18 npts values in the layout tg_jet_load_transform reads (value slots 0);
 * T_out = d^2 psi / d jet(u)^2: 324 npts values, T_ij^{alpha beta} at ((3 i + j) 36 + 6 alpha + beta) npts + q, the layout
 * tg_jet_transform reads with nblk = 9.  Any output may be null; the same subsets give the same bits.
 * A point with |X_,1 x X_,2| or |x_,1 x x_,2| below 1e-14 |X_,1| |X_,2| writes nothing; *nbad counts those points (integer
 * atomics only).  Synchronises the stream.
 * kind 1, params = {mu, thickness, n_thickness} (n_thickness = 1, 2, 3 or 4 as a double): the incompressible neo-Hookean shell of
 * demos/kl-shell-hyper/kl-hyper.py:98-215, psi = sum_k w_k mu/2 (tr C_2D + 1 / det C_2D - 3)(xi_k) with the Gauss rule of
 * n_thickness points on (-h/2, h/2), C_2D = I + R (gm - Gm) R^T from the truncated metrics Gm = A - 2 xi B, gm = a - 2 xi b and
 * the local Cartesian frame of the reference at xi.  Same outputs and layouts; a point is also counted and left alone when
 * det Gm <= 0 or det C_2D <= 0 at one of its thickness points. */
int tg_shell_points(int kind, const double *params, int64_t npts, tg_vec_t Xjet, tg_vec_t ujet, tg_vec_t s_out, tg_vec_t T_out,
                    tg_vec_t psi_out, int64_t *nbad);
/* The follower pressure of kl-hyper.py:231 per unit reference area, -P (x_,1 x x_,2) . v / |X_,1 x X_,2|, ADDED to the outputs of
 * tg_shell_points (same layouts; either may be null): s_i^0 += -P (x_,1 x x_,2)_i / J_A,  T_ij^{0,1} += -(P / J_A) eps_ijk x_,2k,
 * T_ij^{0,2} += (P / J_A) eps_ijk x_,1k -- no transposed entries: the tangent is not symmetric.  A point whose reference normal is
 * below the floor of tg_shell_points is left alone (the law has counted it).  Does not synchronise. */
int tg_shell_pressure_points(int64_t npts, double pressure, tg_vec_t Xjet, tg_vec_t ujet, tg_vec_t s_inout, tg_vec_t T_inout);
/* ---- inertia, mass damping and a rigid-plane penalty at the points (csrc/tg_dynamics.hip): what a dynamic residual adds to the
 * VALUE slots of a law's outputs.  nF = 2, 3 fields of nJ = 1, 3, 6 slots, value slot first (other values: status 2).  u and
 * s_inout: nF nJ npts values, slot alpha of field i at (i nJ + alpha) npts + q (a shell: ujet itself, nJ = 6; a solid: the point
 * values, nJ = 1); T_inout: nF^2 nJ^2 npts values, the value-value entry of block (i, j) at ((i nF + j) nJ^2) npts + q (nJ = 1:
 * the reaction layout of tg_coef_transform_blocks); X0 (reference positions) and w: nF npts values, component-major; e_out:
 * npts values.  coef = {sigma, m_u, m_w, t_m, k_s, k_t, c_e} (host, 7 values), plane = {n[0..nF), offset, unused} (host, nF + 2
 * values; null: no contact, and then X0 may be null):
 *   g = offset - sum_c n_c (X0_c + u_c^0),  g+ = max(g, 0);  a point is active exactly when g > 0
 *   s_i^alpha <- sigma s_i^alpha (every slot; sigma == 1: the bits stay);   s_i^0 += m_u u_i^0 + m_w w_i - k_s g+ n_i
 *   T_ij^00 += delta_ij t_m + k_t [g > 0] n_i n_j   (no other entry of T is read or written)
 *   e_q = c_e/2 sum_i w_i^2 + k_s/2 g+^2
 * Every array may be null (an absent u or w counts as 0); a term with a zero coefficient is not added, so a value it would not
 * change keeps its bits.  *nactive (if given) receives the number of active points: integer atomics only, and the only
 * synchronisation of the call.  No floating-point atomics: the same inputs give the same bits. */
int tg_point_dynamics(int nF, int nJ, int64_t npts, const double *coef, const double *plane, tg_vec_t X0, tg_vec_t u, tg_vec_t w,
                      tg_vec_t s_inout, tg_vec_t T_inout, tg_vec_t e_out, int64_t *nactive);

/* ---- boundary integrals on the same patches (csrc/tg_boundary.hip): the boundary measure and the mapped normal of the
 * reference's ExtractedSpline (spline.ds, spline.n; tIGAr/common.py:931-939, calculusUtils.py:37-52, 71-80).  d = 2, 3,
 * nsd >= d.  A face is (direction dir, side 0 | 1), numbered as getSideDofs; its parametric normal is N = (2 side - 1) e_dir.
 * In reference-element coordinates (g_hat = DF^T DF of the element map, no element size appears), at a face Gauss point
 *   wsurf = w_q sqrt(det g_hat (g_hat^-1)_kk)   (w_q: product of the d-1 tangential Gauss weights; surfaceJacobian times the
 *                                                face element's parametric area)
 *   n     = DF g^-1 N / |DF g^-1 N|             (nsd components)
 *   d_n u = (g^-1 N).grad_xi u / sqrt(N.g^-1 N)
 *   h_n   = 1 / sqrt((g_hat^-1)_kk)             (thickness of the boundary element normal to the face)
 * Points are numbered face-element-major: face elements lexicographic in the remaining directions with the lower
 * direction fastest, the nq^(d-1) points of a face element likewise; npts = nq^(d-1) prod_{j != dir} nel_j.  Arrays with
 * nsd components per point are component-major.  The control functions are given on all FE nodes.  No floating-point
 * atomics (colours over the parities of the tangential element indices): the same inputs give the same bits. */
/* x_q (nsd npts), wsurf_q (npts), n_q (nsd npts), h_n (npts); any output may be null */
int tg_face_points(const tg_patch_t *patch, int dir, int side, tg_vec_t x_out, tg_vec_t wsurf_out, tg_vec_t normal_out,
                   tg_vec_t hn_out);
/* u_h at the face points, its Cartesian gradient (nsd npts) and d_n u_h; grad_out and dn_out may be null */
int tg_face_eval(const tg_patch_t *patch, int dir, int side, tg_vec_t u_nodal, tg_vec_t val_out, tg_vec_t grad_out,
                 tg_vec_t dn_out);
/* out[node] += sum_q wsurf_q (f_q phi_node + fn_q d_n phi_node); either array may be null.  Adds into out: several faces go
 * into one vector.  f_q alone: Neumann / Robin data; both: the Nitsche right-hand side */
int tg_face_load(const tg_patch_t *patch, int dir, int side, tg_vec_t f_q, tg_vec_t fn_q, tg_vec_t out);
/* A_ab = sum_q wsurf_q (a_q phi_a phi_b + b_q phi_a d_n phi_b + c_q d_n phi_a phi_b), each array may be null: an n x n CSR
 * whose non-empty rows are those of the boundary-layer nodes; pattern = the element coupling restricted to the boundary
 * layer, in closed form */
int tg_face_matrix(const tg_patch_t *patch, int dir, int side, tg_vec_t a_q, tg_vec_t b_q, tg_vec_t c_q, tg_csr_t *out);
/* the same entries times `scale`, added in place into A (rows ascending), which must hold them -- every mapped form above
 * does: they return the element-coupling pattern.  Columns by search in the sorted row.  The pattern is checked first: if
 * an entry is missing the call returns 3 and A is unchanged.  A keeps its pattern certificate. */
int tg_face_matrix_add(const tg_patch_t *patch, int dir, int side, tg_vec_t a_q, tg_vec_t b_q, tg_vec_t c_q, double scale,
                       tg_csr_t A);
/* rational twins: u = u_h / W_h, phi -> phi / W_h, grad_xi phi -> (grad_xi phi - phi beta) / W_h */
int tg_face_eval_rational(const tg_patch_t *patch, int dir, int side, tg_vec_t u_nodal, tg_vec_t val_out, tg_vec_t grad_out,
                          tg_vec_t dn_out);
int tg_face_load_rational(const tg_patch_t *patch, int dir, int side, tg_vec_t f_q, tg_vec_t fn_q, tg_vec_t out);
int tg_face_matrix_rational(const tg_patch_t *patch, int dir, int side, tg_vec_t a_q, tg_vec_t b_q, tg_vec_t c_q, tg_csr_t *out);
int tg_face_matrix_add_rational(const tg_patch_t *patch, int dir, int side, tg_vec_t a_q, tg_vec_t b_q, tg_vec_t c_q,
                                double scale, tg_csr_t A);

/* ---- FE operands in the caller's dof order (csrc/tg_feorder.hip, tigar_amd/feorder.py) ----------------------------
 * tg_nodes_locate: recognises the caller's node coordinates x[nrows x d] (host, row-major) as a permutation of the node
 * grid of an FE space of `nfields` scalar fields: field f lives on the tensor grid of the d ascending axes
 * axes[f * d + k] (axis_len[f * d + k] nodes, host), numbered lexicographically with direction 0 fastest, field after
 * field.  field[nrows] (host) names the field of every row; NULL with one field.  Per row every coordinate is snapped to
 * the nearest node of its axis and accepted when the distance is at most tol x (smallest spacing of that axis), 0 <= tol <
 * 0.5; a bijection check on the device follows.  The handle holds grid_of_fe / fe_of_grid (int32, device) and the largest
 * accepted distance.  Status 100 = declined, nothing is kept allocated and tg_last_error names the first offending row
 * and the reason: "off the grid", "two rows on one node", "wrong row count", "node of another field".
 * tg_feorder_from_perm: the handle of a given permutation grid_of_fe[n] (host); 100 when it is none.
 * tg_csr_permute_sym: B = P A P^T, B[g(i), g(j)] = A[i, j] with g = grid_of_fe (inverse != 0: B[i, j] = A[g(i), g(j)]):
 * every row is read once, its columns renamed, sorted by new column on chip and written once; values are copied
 * bit for bit, no atomics on values.  Canonical CSR out.  A must be square and match the handle.
 * tg_vec_permute: y[g(i)] = x[i] (to_caller == 0) or y[i] = x[g(i)] (to_caller != 0); x and y distinct. */
typedef struct tg_feorder_s *tg_feorder_t;
int tg_nodes_locate(int d, int nfields, const int64_t *axis_len, const double *const *axes, const double *x,
                    const int32_t *field, int64_t nrows, double tol, tg_feorder_t *out);
int tg_feorder_from_perm(const int32_t *grid_of_fe, int64_t n, tg_feorder_t *out);
int tg_feorder_info(tg_feorder_t h, int64_t *n, int *identity, double *max_snap);
int tg_feorder_download(tg_feorder_t h, int32_t *grid_of_fe, int32_t *fe_of_grid);
int tg_feorder_destroy(tg_feorder_t h);
int tg_csr_permute_sym(tg_feorder_t h, tg_csr_t a, int inverse, tg_csr_t *out);
int tg_vec_permute(tg_feorder_t h, tg_vec_t x, tg_vec_t y, int to_caller);

/* ---- time integration (csrc/tg_timeint.hip, tigar_amd/timeIntegration.py; tIGAr/timeIntegration.py) ----------------
 * tg_vec_lincomb: out = sum_{i<k} coef[i] v[i] in one pass, 1 <= k <= 8, all of one size; coef and v are host arrays.
 * out may be any of the v[i].  Fixed order (s = coef[0] v[0], then s = fma(coef[i], v[i], s)): same inputs, same bits.
 * tg_state_advance: the state update at the end of a step, in place and in registers:
 *   v = c[0] x + c[1] x_old + c[2] xdot_old + c[3] xddot_old,  a = c[4] v + c[5] xdot_old + c[6] xddot_old,
 *   then x_old = x, xdot_old = v, xddot_old = a.  order == 1: xddot_old is NULL, c[3] and the `a` line are ignored.
 *   c: 7 host doubles.  x is not written; the vectors must be distinct (status 2 otherwise).
 * tg_csr_pair_create: two matrices on ONE sparsity pattern (row pointers and columns compared on the device once;
 *   status 2 when they differ).  The pair borrows the two handles: they must outlive it and keep their pattern.
 * tg_spmv_pair: y = y0 - A xa - B xb; y0 may be NULL (= 0), y may be y0, y must differ from xa and xb.  Every stored
 *   entry is read once: one column, two values (20 B instead of 2 x 12 B), and y is passed over once.  Runs on A's
 *   CSR row-block plan (or a wave per row when a row exceeds it); bit-reproducible. */
typedef struct tg_csr_pair_s *tg_csr_pair_t;
int tg_vec_lincomb(tg_vec_t out, int k, const double *coef, const tg_vec_t *v);
int tg_state_advance(int order, const double *c, tg_vec_t x, tg_vec_t x_old, tg_vec_t xdot_old, tg_vec_t xddot_old);
int tg_csr_pair_create(tg_csr_t A, tg_csr_t B, tg_csr_pair_t *out);
int tg_csr_pair_destroy(tg_csr_pair_t p);
int tg_spmv_pair(tg_csr_pair_t p, tg_vec_t xa, tg_vec_t xb, tg_vec_t y0, tg_vec_t y);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) --------- */
int tg_comm_unique_id(char *id128);                          /* ncclGetUniqueId   */
int tg_comm_create(const char *id128, int rank, int world, tg_comm_t *out);
/* the same with a second RCCL communicator for the halo send/recv pairs (exchange stream), so that they and the
 * all-reduces (solver stream) never share one; id_halo may be NULL.  ncclCommInitRank is given TIGAR_RCCL_TIMEOUT_S
 * seconds (default 180) and reported as failed afterwards instead of blocking for ever. */
int tg_comm_create2(const char *id_reduce128, const char *id_halo128, int rank, int world, tg_comm_t *out);
/* Host-staged communicator: the same solver code, its two exchanges (halo pieces with the z-neighbours,
 * sums of a few doubles over all ranks) staged through pinned host memory and carried by the caller's
 * transport (MPI-style callbacks; 0 = ok).  For process groups RCCL cannot form (ranks sharing a GPU).
 * PETSc counterparts: VecScatter in MatMult, MPI_Allreduce in VecDot/VecNorm (tIGAr/common.py:1255-1258). */
typedef int (*tg_host_allreduce_fn)(void *ctx, double *inout, int n);
typedef int (*tg_host_sendrecv_fn)(void *ctx, int peer, const double *send, int64_t nsend, double *recv,
                                   int64_t nrecv);
int tg_comm_create_host(int rank, int world, tg_host_allreduce_fn allreduce, tg_host_sendrecv_fn sendrecv,
                        void *ctx, tg_comm_t *out);
/* IPC communicator: no host in the loop and no RCCL -- halo planes are pushed by a kernel into the neighbour's device
 * mailbox (hipIpcOpenMemHandle: the same GPU when ranks share one, an xGMI peer otherwise), flags and the slots of
 * the small all-reduce live in the shared file `shm_path` (created and sized to tg_comm_ipc_shm_bytes() zero bytes by
 * the launcher before any rank calls this; at most 16 ranks of one node), waits happen inside the kernels with a
 * wall-clock limit (TIGAR_IPC_TIMEOUT_S, default 60): an exchange is enqueue-only, a dead peer surfaces as an error
 * at the next host wait instead of hanging the GPU.  SURVEY 8(e): "direct xGMI peer copies". */
int tg_comm_ipc_shm_bytes(int64_t *bytes);
int tg_comm_create_ipc(const char *shm_path, int rank, int world, tg_comm_t *out);
int tg_comm_rank_device(tg_comm_t c, int rank, int *device);
/* ranks the communicator really spans (RCCL: ncclCommCount) and its kind (0 = RCCL, 1 = host-staged, 2 = IPC) */
int tg_comm_info(tg_comm_t c, int *rank, int *world, int *kind);
int tg_device_count(int *n);                                 /* visible GPUs      */
/* z-slab descriptor of the Krylov vectors: this rank owns global dofs [g0,g1); the SpMV
 * needs halo_lo dofs below g0 (owned by rank-1) and halo_hi above g1 (rank+1). */
int tg_comm_set_slab(tg_comm_t c, int64_t g0, int64_t g1, int64_t halo_lo, int64_t halo_hi,
                     int64_t nglobal);
int tg_comm_allreduce_sum(tg_comm_t c, double *host_inout, int n);
/* xext = [halo_lo | x_local | halo_hi] with the halos fetched from the z-neighbours */
int tg_comm_halo_extend(tg_comm_t c, tg_vec_t x_local, tg_vec_t xext);
int tg_comm_destroy(tg_comm_t c);
/* one small all-reduce and three halo exchanges with known values on a stream of their own, every host wait bounded by
 * timeout_s: 0 = works; 4 = an exchange did not complete (drop the communicator WITHOUT destroying it); else wrong
 * values / errors.  Collective; the launcher falls back to the next kind of communicator on failure. */
int tg_comm_selftest(tg_comm_t c, double timeout_s);

#ifdef __cplusplus
}
#endif
#endif
