// Cooperative form of the fused posterior kernel (bbh_coop.h), instantiations for small models: n <= 256, i.e. only the last
// four rounds exist (GMIN = 4: half the accumulators, four workgroups per CU), and n <= 128 (GMIN = 6: five).  Matérn-5/2 with and without the task /
// outputscale table, 2 - 8 k-steps of the distance GEMM (d <= 30); with the seeded distance GEMM (KVF bit 8) 2 - 6
// (d <= 24) at n <= 256 and 2, 3 (d <= 12) at n <= 128: the others would not fit the register cap of their occupancy without spilling
// (see below).
#include "bbh_coop.h"

// No instantiation of this kernel may spill: the compiler does not know that a register written by one of the inline-assembly loads
// (operand ring, training fragments) is still in flight until its counted wait, and a spill of such a register between the load
// and the wait saves - and later restores - what the register held BEFORE the load.  At the 96-register cap of five workgroups
// per CU the six-k-step instantiation with the table and both eight-k-step ones spill (12 - 36 bytes); the n <= 128 models with
// that many k-steps therefore run the four-round instantiation (128 registers, four workgroups per CU, no spill).
// SIXV: 0 = four-round instantiation for every n <= 256, 1 = two-round one at n <= 128 without the table only, 2 = with and without
#define BBH_COOP_SMALL_KD_SEL(KDV, SIXV)                                                                    \
  if (kd == KDV) {                                                                                          \
    if (grid.x == 0) return true;                                                                           \
    if constexpr (SIXV == 2) {                                                                              \
      if (a.g0 >= 6 && has_tbl) {                                                                           \
        hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 1, 1, (SIXV == 2 ? 6 : 4)>), grid, dim3(256), lds, s, a); \
        return true;                                                                                        \
      }                                                                                                     \
    }                                                                                                       \
    if constexpr (SIXV >= 1) {                                                                              \
      if (a.g0 >= 6 && !has_tbl) {                                                                          \
        hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 0, 1, (SIXV >= 1 ? 6 : 4)>), grid, dim3(256), lds, s, a); \
        return true;                                                                                        \
      }                                                                                                     \
    }                                                                                                       \
    if (has_tbl)                                                                                            \
      hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 1, 1, 4>), grid, dim3(256), lds, s, a);             \
    else                                                                                                    \
      hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 0, 1, 4>), grid, dim3(256), lds, s, a);             \
    return true;                                                                                            \
  }

bool bbh_coop_launch_small(int kd, int kind, bool has_tbl, dim3 grid, size_t lds, hipStream_t s, const CoopArgs& a) {
  if (kind != BBH_KERNEL_MATERN52) return false;
  BBH_COOP_SMALL_KD_SEL(2, 2)
  BBH_COOP_SMALL_KD_SEL(4, 2)
  BBH_COOP_SMALL_KD_SEL(6, 1)
  BBH_COOP_SMALL_KD_SEL(8, 0)
  return false;
}

#define BBH_COOP_SMALL_SEED_KD(KDV)                                                                         \
  if (kds == KDV) {                                                                                         \
    if (grid.x == 0) return true;                                                                           \
    if (a.g0 >= 6 && has_tbl) /* n <= 128 */                                                                \
      hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 9, 1, 6>), grid, dim3(256), lds, s, a);             \
    else if (a.g0 >= 6)                                                                                     \
      hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 8, 1, 6>), grid, dim3(256), lds, s, a);             \
    else if (has_tbl)                                                                                       \
      hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 9, 1, 4>), grid, dim3(256), lds, s, a);             \
    else                                                                                                    \
      hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 8, 1, 4>), grid, dim3(256), lds, s, a);             \
    return true;                                                                                            \
  }
// 128 < n <= 256 only: false at n <= 128, where the caller keeps the augmented stream's instantiation
#define BBH_COOP_SMALL_SEED_KD4(KDV)                                                                        \
  if (kds == KDV) {                                                                                         \
    if (a.g0 >= 6) return false;                                                                            \
    if (grid.x == 0) return true;                                                                           \
    if (has_tbl)                                                                                            \
      hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 9, 1, 4>), grid, dim3(256), lds, s, a);             \
    else                                                                                                    \
      hipLaunchKernelGGL((bbh_coop_posterior_kernel<KDV, 8, 1, 4>), grid, dim3(256), lds, s, a);             \
    return true;                                                                                            \
  }

// (a.g0 decides also when grid.x == 0 only asks)
bool bbh_coop_seed_launch_small(int kds, bool has_tbl, dim3 grid, size_t lds, hipStream_t s, const CoopArgs& a) {
  BBH_COOP_SMALL_SEED_KD(2)
  BBH_COOP_SMALL_SEED_KD(3)
  BBH_COOP_SMALL_SEED_KD4(4)
  BBH_COOP_SMALL_SEED_KD4(5)
  BBH_COOP_SMALL_SEED_KD4(6)
  return false;
}
