// Cooperative form of the fused posterior kernel (bbh_coop.h) with the seeded distance GEMM: the training-fragment stream
// without the two augmentation rows, ceil(d / 4) k-steps (2 - 8 and 12: d <= 32 and d = 47, 48 - wherever that is fewer k-steps
// than the augmented stream's instantiation has), Matérn-5/2 with and without the task / outputscale table; and the dispatcher
// over this translation unit and the small-model instantiations.
#include "bbh_coop.h"

#define BBH_COOP_SEED_KD(KDV)                                                                \
  if (kds == KDV) {                                                                          \
    if (grid.x == 0) return true;                                                            \
    if (has_tbl)                                                                             \
      hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 9, 1>), grid, dim3(256), lds, s, a); \
    else                                                                                     \
      hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 8, 1>), grid, dim3(256), lds, s, a); \
    return true;                                                                             \
  }

bool bbh_coop_seed_launch(int kds, bool has_tbl, dim3 grid, size_t lds, hipStream_t s, const CoopArgs& a, bool small_ok) {
  if (grid.x != 0 && a.g0 >= 4 && small_ok && bbh_coop_seed_launch_small(kds, has_tbl, grid, lds, s, a)) return true;
  BBH_COOP_SEED_KD(2)
  BBH_COOP_SEED_KD(3)
  BBH_COOP_SEED_KD(4)
  BBH_COOP_SEED_KD(5)
  BBH_COOP_SEED_KD(6)
  BBH_COOP_SEED_KD(7)
  BBH_COOP_SEED_KD(8)
  BBH_COOP_SEED_KD(12)
  return false;
}
