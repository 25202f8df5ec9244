// bamsplit.hip -- the round-2 region split and the query-name suffix on the BAM session (SURVEY.md §8f rows f4b and
// f6b).
//
// Replaces the record loops of filter_and_split_reads_by_region (ont_tcr_consensus/region_split.py:336-435) and of
// estimate_precision_at_num_subreads (minimap2_align.py:362-435).  Both read the filtered consensus BAM, which the
// session (bamscan.hip) has scanned already: k_split_cols classifies a record from the session's columns (class,
// refID, l_seq, reference_length) with k_bam_classify's decision chain (bam_bounds.h) and never walks a CIGAR again; the FASTA
// bytes of the kept records are k_bam_emit's (regionsplit.hip), unchanged.  k_name_suffix parses the decimal field
// after the last "_" of every query name.  One thread per record, a few bytes each: launch-bound, no LDS, no atomics.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "bam_bounds.h"
#include "bam_host.h"
#include "umiclust_internal.h"

namespace uc {

// per record: class (kBamUnmapped ... kBamAbsent), bucket, output bytes.  keep: null = every record is in the file
__global__ void k_split_cols(const BamScanCols o, const uint8_t* __restrict__ raw, const int64_t* __restrict__ roff,
                             const uint8_t* __restrict__ keep, int64_t n, int32_t nref,
                             const int64_t* __restrict__ ref_len, const int32_t* __restrict__ ref_bucket, double minov,
                             int32_t s5, int32_t s3, int8_t* __restrict__ cls, int32_t* __restrict__ bucket,
                             int64_t* __restrict__ outlen) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int8_t scan = o.cls[r];
  const int32_t ref = o.ref[r], lseq = o.l_seq[r];
  int8_t c;
  int32_t k = -1;
  int64_t len = 0;
  if (keep && !keep[r]) {
    c = kBamAbsent;
  } else if (scan == bam::kScanUnmapped) {
    c = kBamUnmapped;
  } else if (scan == bam::kScanSecondary) {
    c = kBamSecondary;
  } else {
    const uint32_t lrn = bam::l_read_name(raw + roff[r]);  // the host refuses a kept record with 0
    region_class(ref, nref, ref_len, ref_bucket, o.reflen[r], lseq, lrn, minov, s5 + s3, c, k, len);
  }
  cls[r] = c;
  bucket[r] = k;
  outlen[r] = len;
}

// per record: the query name's tail (what follows its last '_', or the whole name) as a decimal value.  status 1: the
// tail is 1..18 ASCII digits; 0: anything else (empty, a sign, a non-digit, 19 digits or more), which is left to
// Python's int().  Reads backwards from the name's last byte, at most 19 bytes, all inside the record.
__global__ void k_name_suffix(const uint8_t* __restrict__ raw, const int64_t* __restrict__ roff, int64_t n,
                              int64_t* __restrict__ value, uint8_t* __restrict__ status) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint8_t* rec = raw + roff[r];
  const uint32_t room = bam::block_size(rec) - 32, lrn = bam::l_read_name(rec);  // record_offsets: block_size >= 32
  int len = (int)(lrn < room ? lrn : room);
  const uint8_t* name = bam::name(rec);
  if (len && name[len - 1] == 0) len--;
  int64_t v = 0, mul = 1;
  int nd = 0;
  bool ok = true;
  for (int k = 0; k < 19; k++) {
    const int x = len - 1 - k;
    if (x < 0) break;
    const uint8_t ch = name[x];
    if (ch == '_') break;
    if (ch < '0' || ch > '9' || k == 18) {
      ok = false;
      break;
    }
    v += (int64_t)(ch - '0') * mul;
    mul *= 10;
    nd++;
  }
  ok = ok && nd > 0;
  value[r] = ok ? v : 0;
  status[r] = ok ? 1 : 0;
}

hipError_t launch_split_cols(const BamScanCols& o, const uint8_t* raw, const int64_t* roff, const uint8_t* keep,
                             int64_t n, int32_t nref, const int64_t* ref_len, const int32_t* ref_bucket, double minov,
                             int32_t s5, int32_t s3, int8_t* cls, int32_t* bucket, int64_t* outlen, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_split_cols, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, o, raw, roff, keep, n, nref,
                     ref_len, ref_bucket, minov, s5, s3, cls, bucket, outlen);
  return hipGetLastError();
}

hipError_t launch_name_suffix(const uint8_t* raw, const int64_t* roff, int64_t n, int64_t* value, uint8_t* status,
                              hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_name_suffix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, raw, roff, n, value, status);
  return hipGetLastError();
}

}  // namespace uc
