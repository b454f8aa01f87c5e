// Host emulation of the z walk of the tensor-pattern PtAP that holds the last B2 block of every node slot in registers
// (tigar_amd/csrc/tg_tensor_body.h: tt_z_lane<P, true>, tt_z_held), lane by lane, beside the plain walk tt_z_lane<P>.
// Test infrastructure only (CPU suite, tests/test_z_cache_emulation.py).  Built as a shared library for the Python test;
// with -DZ_CACHE_EMU_MAIN it is a stand-alone program (its own cases, plain walk on copies against the holding walk on
// shared blocks, exit status 0 when every K is equal bit for bit) that can run under the host sanitizers.
#include "../../tigar_amd/csrc/tg_tensor_body.h"
#include <stdint.h>

template <int P, bool C>
static void run_z(const tt_z_args &A, int gx) {
  for (int bx = 0; bx < gx; bx++)
    for (int lane = 0; lane < 64; lane++) tt_z_lane<P, C>(A, bx, lane);
}

extern "C" {
// one z stage over the dof planes [ka, kb); held != 0: the block-holding walk
void emu_zc(int held, int P, const double *const *planes, int plane_lo, int nel2, const double *wl2, const int32_t *kps2,
            int ncp0, int ncp1, const int32_t *kps0, const int32_t *kps1, int ka, int kb, int L, int32_t *kcol, double *kval,
            const uint8_t *mask, double diag) {
  tt_z_args A = {};
  A.planes = planes;
  A.plane_lo = plane_lo;
  A.d2.nel = nel2;
  A.d2.nfe = P * nel2 + 1;
  A.d2.ncp = nel2 + P;
  A.d2.wl = wl2;
  A.d2.kps = kps2;
  A.ncp0 = ncp0;
  A.ncp1 = ncp1;
  A.kps0 = kps0;
  A.kps1 = kps1;
  A.ka = ka;
  A.kb = kb;
  A.L = L;
  A.kcol = kcol;
  A.kval = kval;
  A.mask = mask;
  A.diag = diag;
  const int gx = (int)(((int64_t)ncp0 * ncp1 + L - 1) / L);
  if (P == 1) held ? run_z<1, true>(A, gx) : run_z<1, false>(A, gx);
  else if (P == 2) held ? run_z<2, true>(A, gx) : run_z<2, false>(A, gx);
  else held ? run_z<3, true>(A, gx) : run_z<3, false>(A, gx);
}

// what the host decides and counts from the pointer table of a stage (tg_tensor_zstage)
int emu_z_repeats(int P, const double *const *ptr, int n) { return tt_z_repeats(P, ptr, n) ? 1 : 0; }
int emu_z_block_loads(int P, int plo, int nfe, const double *const *ptr, int n, int held) {
  return tt_z_block_loads(P, plo, nfe, ptr, n, held != 0);
}
}  // extern "C"

#ifdef Z_CACHE_EMU_MAIN
#include <stdio.h>

namespace {
uint64_t g_state = 0x9e3779b97f4a7c15ull;
double rnd() {   // xorshift64*, values in [-1, 1)
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (double)((g_state * 2685821657736338717ull) >> 11) / 4503599627370496.0 - 1.0;
}
std::vector<int32_t> widths_ps(int nel, int P) {
  const int ncp = nel + P;
  std::vector<int32_t> kps((size_t)ncp + 1, 0);
  for (int i = 0; i < ncp; i++) kps[(size_t)i + 1] = kps[(size_t)i] + (std::min(ncp - 1, i + P) - std::max(0, i - P) + 1);
  return kps;
}

// classes 0: first plane, 1: last plane, 2..P: nodes inside an element, P + 1: vertices; kind 0: these (uniform knots), 1: every
// plane its own class, 2: uniform on the first half, 3: uniform on the second half, 4: uniform data, but every second element
// keeps copies of its own (equal data behind other pointers at stride P)
int run_case(int P, int nel2, int kind, bool with_mask) {
  const int W = 2 * P + 1, nfe2 = P * nel2 + 1, ncp2 = nel2 + P, ncp0 = P + 2, ncp1 = P + 1;
  const std::vector<int32_t> kps0 = widths_ps(ncp0 - P, P), kps1 = widths_ps(ncp1 - P, P), kps2 = widths_ps(nel2, P);
  std::vector<double> wl((size_t)nel2 * (P + 1) * (P + 1));
  for (double &w : wl) w = rnd();
  std::vector<int> cls((size_t)nfe2), grp((size_t)nfe2);
  for (int a = 0; a < nfe2; a++) {
    const int u = a == 0 ? 0 : a == nfe2 - 1 ? 1 : a % P ? 1 + a % P : P + 1;
    const bool uni = kind == 0 || kind == 4 || (kind == 2 && a < nfe2 / 2) || (kind == 3 && a >= nfe2 / 2);
    cls[(size_t)a] = uni ? u : P + 2 + a;
    grp[(size_t)a] = kind == 4 && ((a - 1) / P) % 2 ? 1000 + a : cls[(size_t)a];
  }
  std::vector<std::vector<double>> own((size_t)nfe2), shared((size_t)nfe2);   // reference copies; one block per group (at its first plane)
  std::vector<const double *> pref((size_t)nfe2), pali((size_t)nfe2);
  for (int a = 0; a < nfe2; a++) {
    const int n2 = (a % P == 0 && a > 0 && a < nfe2 - 1) ? W : P + 1;
    const size_t len = (size_t)W * W * n2 * ncp0 * ncp1;
    int first = a, gfirst = a;
    for (int b = a - 1; b >= 0; b--) {
      if (cls[(size_t)b] == cls[(size_t)a]) first = b;
      if (grp[(size_t)b] == grp[(size_t)a]) gfirst = b;
    }
    own[(size_t)a].resize(len);
    if (first == a)
      for (double &v : own[(size_t)a]) v = rnd();
    else
      own[(size_t)a] = own[(size_t)first];
    if (gfirst == a) shared[(size_t)a] = own[(size_t)a];
    pref[(size_t)a] = own[(size_t)a].data();
    pali[(size_t)a] = shared[(size_t)gfirst].data();
  }
  const int64_t ntot = (int64_t)ncp0 * ncp1 * ncp2;
  std::vector<uint8_t> mask((size_t)ntot, 0);
  for (uint8_t &m : mask) m = rnd() > 0.4 ? 1 : 0;
  const int64_t w01 = (int64_t)kps0[(size_t)ncp0] * kps1[(size_t)ncp1];
  const int64_t nnz = w01 * kps2[(size_t)ncp2];
  int bad = 0;
  for (int cut = 0; cut <= ncp2; cut++) {                 // cut 0: one stage; ncp2: single dof planes; else two sub-slabs
    std::vector<int> edges;
    if (cut == 0) edges = {0, ncp2};
    else if (cut == ncp2)
      for (int i = 0; i <= ncp2; i++) edges.push_back(i);
    else edges = {0, cut, ncp2};
    std::vector<int32_t> col[2];
    std::vector<double> val[2];
    for (int h = 0; h < 2; h++) {
      col[h].assign((size_t)nnz, -1);
      val[h].assign((size_t)nnz, 0.0);
      int64_t at = 0;
      for (size_t s = 0; s + 1 < edges.size(); s++) {
        const int ka = edges[s], kb = edges[s + 1];
        const int e_begin = std::max(0, ka - P);
        const int plo = e_begin == 0 ? 0 : P * e_begin + 1;
        const std::vector<const double *> &tab = h ? pali : pref;
        emu_zc(h, P, tab.data() + plo, plo, nel2, wl.data(), kps2.data(), ncp0, ncp1, kps0.data(), kps1.data(), ka, kb,
               std::max(1, 64 / (W * W)), col[h].data() + at, val[h].data() + at, with_mask ? mask.data() : nullptr, 2.5);
        at += w01 * (kps2[(size_t)kb] - kps2[(size_t)ka]);
      }
    }
    if (col[0] != col[1] || memcmp(val[0].data(), val[1].data(), (size_t)nnz * sizeof(double)) != 0) bad++;
    for (int32_t c : col[1])
      if (c < 0) bad++;
  }
  return bad;
}
}  // namespace

int main() {
  int bad = 0, n = 0;
  const int nel2s[4] = {1, 2, 5, 8};
  for (int P = 1; P <= 3; P++)
    for (int nel2 : nel2s)
      for (int kind = 0; kind < 5; kind++)
        for (int m = 0; m < 2; m++) {
          bad += run_case(P, nel2, kind, m != 0);
          n++;
        }
  printf("z_cache_emu: %d cases, %d mismatches\n", n, bad);
  return bad ? 1 : 0;
}
#endif
