// Host build of the plane-class partition of the tensor-pattern PtAP (tt_plane_classes in
// tigar_amd/csrc/tg_tensor_body.h): the very function the native driver calls before the x and y passes of a
// Kronecker-sum form.  Test infrastructure only (CPU suite).  Not part of the product library.
#include "../../tigar_amd/csrc/tg_tensor_body.h"
#include <stdint.h>

extern "C" {
// rep[q - z0] = lowest plane of [z0, z1) whose row of the last-direction factor equals that of plane q; returns the
// number of classes
int emu_plane_classes(int nterms, int64_t nnz, const double *val, const int32_t *rps, int z0, int z1, int32_t *rep) {
  return tt_plane_classes(nterms, nnz, val, rps, z0, z1, rep);
}
}
