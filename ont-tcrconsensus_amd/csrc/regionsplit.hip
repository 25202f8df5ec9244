// regionsplit.hip -- region binning of aligned reads on the GPU.
//
// Replaces the per-record loop of filter_and_split_reads_by_region_cluster
// (/root/reference/ont_tcr_consensus/region_split.py:219-333), which sets the shard sizes of the clustering
// hot path: every BAM record is classified (unmapped / secondary or supplementary / too short an overlap /
// too long / kept) and every kept read is written to region_cluster<k>.fasta as
// `>{query_name};strand={+|-}` + its forward sequence (pysam get_forward_sequence: reverse-complemented for
// reverse-strand records).  The BGZF blocks are inflated on the device (bgzf.hip) and the host finds the record
// offsets; on the device one thread per record decodes the fixed fields and the CIGAR (reference_length =
// M/D/N/=/X lengths) and classifies it, and one wave per kept record writes its FASTA bytes -- the 4-bit
// sequence decoded (and reverse-complemented) lane-parallel -- at its slot in a cluster-grouped output
// buffer, which the host appends to the cluster files.  Byte work: HBM/PCIe-bound, no MFMA.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "bam_bounds.h"
#include "bam_record.h"
#include "umiclust_internal.h"

namespace uc {

// region_class, the decision chain on a primary record (:261-271), with long_bound, the `too long` bound as the
// reference rounds it (:264-267): bam_bounds.h

// per record: class (kBamUnmapped ... kBamNoCluster), cluster, output bytes
__global__ void k_bam_classify(const uint8_t* __restrict__ raw, const int64_t* __restrict__ roff, int64_t n,
                               int32_t nref, const int64_t* __restrict__ ref_len, const int32_t* __restrict__ ref_cluster,
                               double minov, int32_t s5, int32_t s3, int8_t* __restrict__ cls,
                               int32_t* __restrict__ cluster, int64_t* __restrict__ outlen) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint8_t* rec = raw + roff[r];
  const int32_t ref = bam::ref_id(rec);
  const uint32_t lrn = bam::l_read_name(rec), ncig = bam::n_cigar_op(rec), flag = bam::flag(rec);
  const int32_t lseq = bam::l_seq(rec);
  int8_t c;
  int32_t k = -1;
  int64_t len = 0;
  if (flag & bam::kFlagUnmapped) {
    c = kBamUnmapped;
  } else if (flag & bam::kFlagNotPrimary) {
    c = kBamSecondary;
  } else {
    const uint8_t* cg = bam::cigar(rec, lrn);
    int64_t rl = 0;
    for (uint32_t x = 0; x < ncig; x++) {
      const uint32_t v = bam::le32(cg + 4 * x);
      if (bam::op_on_reference(v & 15u)) rl += v >> 4;
    }
    // pysam's reference_length = bam_endpos - pos: a record without a reference span is 1 base long and drops as
    // short (:261-263)
    rl = bam::reference_span(rl);
    region_class(ref, nref, ref_len, ref_cluster, rl, lseq, lrn, minov, s5 + s3, c, k, len);
  }
  cls[r] = c;
  cluster[r] = k;
  outlen[r] = len;
}

// one wave per kept record: ">{name};strand={s}\n{forward sequence}\n" at pos[r]
__global__ void k_bam_emit(const uint8_t* __restrict__ raw, const int64_t* __restrict__ roff, int64_t n,
                           const int8_t* __restrict__ cls, const int64_t* __restrict__ pos, char* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n || cls[r] != kBamKept) return;
  const uint8_t* rec = raw + roff[r];
  const uint32_t lrn = bam::l_read_name(rec), ncig = bam::n_cigar_op(rec), flag = bam::flag(rec);
  const int32_t lseq = bam::l_seq(rec);
  const uint8_t* name = bam::name(rec);
  const uint8_t* sq = bam::seq(rec, lrn, ncig);
  char* o = out + pos[r];
  const int nl = (int)lrn - 1;
  for (int x = lane; x < nl; x += 64) o[1 + x] = (char)name[x];
  if (lane == 0) {
    o[0] = '>';
    const char* tag = ";strand=";
    for (int x = 0; x < 8; x++) o[1 + nl + x] = tag[x];
    o[1 + nl + 8] = (flag & bam::kFlagReverse) ? '-' : '+';
    o[1 + nl + 9] = '\n';
  }
  char* s = o + 1 + nl + 10;
  if (lseq <= 0) {
    if (lane < 4) s[lane] = "None"[lane];
    if (lane == 0) s[4] = '\n';
    return;
  }
  const bool rev = (flag & bam::kFlagReverse) != 0;
  for (int x = lane; x < lseq; x += 64) s[x] = bam::forward_base(sq, lseq, rev, x);
  if (lane == 0) s[lseq] = '\n';
}

hipError_t launch_bam_classify(const uint8_t* raw, const int64_t* roff, int64_t n, int32_t nref, const int64_t* ref_len,
                               const int32_t* ref_cluster, double minov, int32_t s5, int32_t s3, int8_t* cls,
                               int32_t* cluster, int64_t* outlen, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bam_classify, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, raw, roff, n, nref, ref_len,
                     ref_cluster, minov, s5, s3, cls, cluster, outlen);
  return hipGetLastError();
}

hipError_t launch_bam_emit(const uint8_t* raw, const int64_t* roff, int64_t n, const int8_t* cls, const int64_t* pos,
                           char* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bam_emit, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, raw, roff, n, cls, pos, out);
  return hipGetLastError();
}

}  // namespace uc
