// bam_bounds.h -- the decision chain of the region filters on one primary record, shared by k_bam_classify
// (regionsplit.hip, row f4) and k_split_cols (bamsplit.hip, row f4b), and its `too long` bound.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "umiclust_internal.h"

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

// A mapped primary record on reference `ref`, with reference_length `reflen`: its class (kBamNoRegion, kBamShort,
// kBamLong, kBamNoCluster or kBamKept) and, for a kept one, its bucket and the bytes of ">name;strand=s\nSEQ\n" (SEQ
// is "None" without a sequence).  lrn: l_read_name, with the NUL.  The zero guard on it is for k_split_cols, whose
// host refuses a kept record with l_read_name 0 only afterwards; k_bam_classify is never launched on one, because
// bam::check_record_fields refuses l_read_name < 1 first, so the guard cannot change its results.
__device__ __forceinline__ void region_class(int32_t ref, int32_t nref, const int64_t* __restrict__ ref_len,
                                             const int32_t* __restrict__ ref_bucket, int64_t reflen, int32_t lseq,
                                             uint32_t lrn, double minov, int32_t slack, int8_t& c, int32_t& bucket,
                                             int64_t& outlen) {
  bucket = -1, outlen = 0;
  if (ref < 0 || ref >= nref || ref_len[ref] < 0) {
    c = kBamNoRegion;  // region_length_dict[entry.reference_name] raises
    return;
  }
  const double L = (double)ref_len[ref];
  const double bound = long_bound(L, minov, slack);
  if ((double)reflen < L * minov) {
    c = kBamShort;
  } else if ((double)lseq > bound) {
    c = kBamLong;
  } else if (ref_bucket[ref] < 0) {
    c = kBamNoCluster;  // region_cluster_dict[entry.reference_name] raises
  } else {
    c = kBamKept;
    bucket = ref_bucket[ref];
    outlen = 1 + (int64_t)(lrn ? lrn - 1 : 0) + 9 + 1 + (lseq > 0 ? lseq : 4) + 1;
  }
}

}  // namespace uc
