// bam_bounds.h -- the `too long` bound of the region filters, shared by k_bam_classify (regionsplit.hip, row f4) and
// k_split_cols (bamsplit.hip, row f4b).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace uc {

// region_length * (2 - minimal_region_overlap) + (max_softclip_5_end + max_softclip_3_end) as the reference evaluates
// it (region_split.py:264-267 and :377-380): the product rounded to a double, then the add.  Contracted into one fma
// (the compiler's default, and __dmul_rn / __dadd_rn do not prevent it) the bound can land one ulp lower, and a read
// exactly at it drops as long: region 400, overlap 0.93, slack 141 gives 569.0 rounded and 568.9999999999999 fused.
__device__ __forceinline__ double long_bound(double L, double minov, int32_t slack) {
#pragma clang fp contract(off)
  const double prod = L * (2.0 - minov);
  return prod + (double)slack;
}

}  // namespace uc
