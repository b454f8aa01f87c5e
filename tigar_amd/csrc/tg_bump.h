// The host side of a bump-allocating PtAP pass, once: the kernel reserves its rows in a temporary
// with a cursor (or at a fixed stride) and reports a status; the host grows whatever overflowed and launches again; a scan
// and the row-reorder copy then turn the temporary into CSR, and the scanned counts are the pattern remembered for the
// next product.  The kernels, their launches and their growth rules stay with the sites (tg_ptap.hip, tg_ptap_wave.hip,
// tg_ptap_box.hip).
#pragma once
#include "tg_common.h"

// what a site's growth rule answers besides a return code (> 0); run() returns TG_BUMP_NORUN when an attempt did not run
// (the site words the error) and TG_BUMP_RETRY when the last attempt still asked for another one
enum { TG_BUMP_DONE = 0, TG_BUMP_RETRY = -1, TG_BUMP_NORUN = -2 };

struct tg_bump {
  const char *site;             // names the pass in the trace
  int64_t nrows = 0, capacity = 0;
  int ts[2] = {0, 0};           // the site's table sizes (trace only)
  int nstatus = 3;              // status words at g_tg.scratch that an attempt zeroes and reads back (<= 4)
  int ncursor = 0;              // words of the cursor (0: rows at a fixed stride only)
  tg_dbuf<int64_t> cnt, off;    // entries per row (null: the site keeps its own), start of every row in the temporary
  tg_dbuf<unsigned long long> cursor;
  tg_dbuf<int32_t> tcol;
  tg_dbuf<double> tval;
  unsigned long long used = 0;  // the cursor after the last attempt

  explicit tg_bump(const char *site_) : site(site_) {}
  int *status() const { return (int *)g_tg.scratch; }

  int init(int64_t nrows_, bool with_cnt, int ncursor_, int nstatus_) {
    nrows = nrows_;
    ncursor = ncursor_;
    nstatus = nstatus_;
    if (with_cnt) TG_TRY(cnt.alloc(nrows + 1));
    TG_TRY(off.alloc(nrows + 1));
    if (ncursor) TG_TRY(cursor.alloc(ncursor));
    return 0;
  }

  // a temporary of `cap` entries (the old one goes back to the pool first) and everything an attempt starts from zeroed
  int reserve(int64_t cap) {
    tcol.reset();
    tval.reset();
    capacity = cap;
    TG_TRY(tcol.alloc(cap + TG_CSR_PAD));
    TG_TRY(tval.alloc(cap + TG_CSR_PAD));
    TG_CHECK_HIP(hipMemsetAsync(status(), 0, (size_t)nstatus * sizeof(int), g_tg.stream));
    if (cursor) TG_CHECK_HIP(hipMemsetAsync(cursor, 0, (size_t)ncursor * sizeof(unsigned long long), g_tg.stream));
    if (cnt) TG_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)(nrows + 1) * sizeof(int64_t), g_tg.stream));
    return 0;
  }

  // launch(attempt): issues the site's kernel on the temporary reserved for `capacity` (a return code ends the pass);
  // decide(attempt, status words, used): TG_BUMP_DONE, TG_BUMP_RETRY after growing `capacity` / the tables, or a return code
  template <typename Launch, typename Decide>
  int run(int max_attempts, Launch launch, Decide decide) {
    const bool trace = getenv("TIGAR_TRACE") != nullptr;
    int verdict = TG_BUMP_RETRY;
    for (int attempt = 0; attempt < max_attempts && verdict == TG_BUMP_RETRY; attempt++) {
      TG_TRY(reserve(capacity));
      TG_TRY(launch(attempt));
      int h[4] = {0, 0, 0, 0};
      used = 0;
      bool ran = hipMemcpyAsync(h, status(), (size_t)nstatus * sizeof(int), hipMemcpyDeviceToHost, g_tg.stream) == hipSuccess;
      if (ran && cursor) ran = hipMemcpyAsync(&used, cursor, sizeof(used), hipMemcpyDeviceToHost, g_tg.stream) == hipSuccess;
      if (hipStreamSynchronize(g_tg.stream) != hipSuccess || hipGetLastError() != hipSuccess || !ran) return TG_BUMP_NORUN;
      const long long cap = (long long)capacity;
      const int t0 = ts[0], t1 = ts[1];
      verdict = decide(attempt, (const int *)h, used);
      if (trace)
        fprintf(stderr, "[tigar] ptap temporary (%s): attempt %d status %d used %llu capacity %lld tables %d / %d -> %s\n", site,
                attempt, h[0], used, cap, t0, t1, verdict == TG_BUMP_DONE ? "done" : verdict == TG_BUMP_RETRY ? "retry" : "gave up");
      if (verdict != TG_BUMP_DONE) {
        tcol.reset();
        tval.reset();
      }
    }
    return verdict;
  }

  // scan of the counts, a CSR of its own, rows into order.  *k is set as soon as it exists (the caller destroys it on
  // error); keep / keep_nnz (or null): receive the scanned counts -- the row pointer of K -- as the pattern to remember
  int finish_csr(const char *who, int64_t ncols, tg_csr_s **k, int64_t **keep, int64_t *keep_nnz) {
    int64_t nnz = 0;
    TG_TRY(tg_exclusive_scan_i64(cnt, nrows, &nnz));
    TG_TRY(tg_csr_alloc(nrows, ncols, nnz, k));
    TG_CHECK_HIP(hipMemcpyAsync((*k)->rowptr, cnt, (size_t)(nrows + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, g_tg.stream));
    TG_TRY(tg_rows_reorder(who, (*k)->rowptr, off, nullptr, tcol, tval, nrows, (*k)->col, (*k)->val));
    if (keep) {
      tg_dfree(*keep);
      *keep = cnt.release();
      *keep_nnz = nnz;
    }
    return 0;
  }
};
