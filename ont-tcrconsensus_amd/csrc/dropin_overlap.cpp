// dropin_overlap.cpp -- region overlap (§8f f3): the host side of csrc/overlap.hip on the context core (ctx.h).
#include <vector>

#include "ctx.h"

using namespace uc;

void uc::overlap_table(Ctx* c, OvRun& R, const char* seqs, const int64_t* offs, int64_t n, const int64_t* rstart,
                       int32_t nreg, bool csr, int hash_bits) {
  if (n < 0 || nreg < 1 || (n > 0 && (!seqs || !offs)) || !rstart) c->fail(UMICLUST_EINVAL, "null argument");
  if (rstart[0] != 0 || rstart[nreg] != n) c->fail(UMICLUST_EINVAL, "region boundaries must span [0, n]");
  for (int32_t r = 0; r < nreg; r++)
    if (rstart[r + 1] < rstart[r]) c->fail(UMICLUST_EINVAL, "region boundaries must not decrease");
  if (n > (int64_t)UINT32_MAX / 2) c->fail(UMICLUST_ERANGE, "too many sequences");
  uint64_t m = 1024;
  while (m < (uint64_t)(2 * n)) m <<= 1;
  R.mask = m - 1;
  c->hip(R.d_rs.ensure((size_t)nreg + 1), "alloc");
  alloc_each(c, (size_t)n + 1, R.d_slot, R.d_hash, R.d_reg, R.d_members);
  alloc_each(c, m, R.d_keys, R.d_rep, R.d_cnt, R.d_cursor);
  c->hip(R.d_start.ensure(m + 1), "alloc");
  c->hip(R.d_bsum.ensure(m / 1024 + 1), "alloc");
  c->hip(R.d_big.ensure((size_t)n / (kOvSmallBucket + 1) + 1), "alloc");
  alloc_each(c, 1, R.d_coll, R.d_nbig);
  std::vector<int64_t> rel;  // read by the offset copy: every table pass below ends with a stream synchronisation
  upload_seqs(c, seqs, offs, n, R.d_seq, R.d_off, rel, c->st);
  c->hip(hipMemcpyAsync(R.d_rs.p, rstart, ((size_t)nreg + 1) * 8, hipMemcpyHostToDevice, c->st), "h2d");
  R.B = OvBuffers{R.d_hash.p, R.d_reg.p, R.d_keys.p, R.d_rep.p, R.d_slot.p, R.d_cnt.p, R.d_start.p, R.d_cursor.p,
                  R.d_bsum.p, R.d_members.p, R.d_coll.p, R.d_big.p, R.d_nbig.p};
  // a 64-bit collision between two different sequences is detected exactly; the next seed is tried
  const uint64_t seeds[4] = {0x243f6a8885a308d3ull, 0x13198a2e03707344ull, 0xa4093822299f31d0ull,
                             0x082efa98ec4e6c89ull};
  // first pass: 8-bit hashes under UMICLUST_OVERLAP_TEST_COLLIDE, hash_bits of them where the probe asks for fewer
  if (hash_bits == 64 && env_overlap_test_collide()) hash_bits = 8;
  const uint64_t first = hash_bits < 64 ? (1ull << hash_bits) - 1 : ~0ull;
  R.passes = 0;
  for (int k = 0; k < 4; k++) {
    uint32_t coll = 0;
    const uint64_t hmask = k == 0 ? first : ~0ull;
    c->hip(launch_overlap_table(R.d_seq.p, R.d_off.p, n, R.d_rs.p, nreg, seeds[k], hmask, R.mask, R.B, csr, &coll,
                                c->st),
           "overlap table");
    c->stats.n_overlap_passes++;
    R.passes++;
    R.seed = seeds[k];
    if (!coll) return;
  }
  c->fail(UMICLUST_EDEVICE, "overlap: 64-bit hash collisions under four seeds");
}

int32_t umiclust_overlap_counts(umiclust_ctx* ctx, const char* s1, const int64_t* off1, int64_t n1, const char* s2,
                                const int64_t* off2, int64_t n2, int64_t* counts) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (n1 < 0 || n2 < 0 || (n1 > 0 && (!s1 || !off1 || !counts)) || (n2 > 0 && (!s2 || !off2)))
      c->fail(UMICLUST_EINVAL, "null argument");
    // one buffer: set 1 then set 2
    std::vector<char> all;
    std::vector<int64_t> off{0};
    append_set(s1, off1, n1, all, off);
    append_set(s2, off2, n2, all, off);
    const int64_t n = n1 + n2, rs[3] = {0, n1, n};
    OvRun R;
    overlap_table(c, R, all.data(), off.data(), n, rs, 2, false);
    DevBuf<int64_t> d_counts;
    c->hip(d_counts.ensure((size_t)n1 + 1), "alloc");
    c->hip(launch_overlap_two(R.B, R.mask, n, n1, d_counts.p, c->st), "overlap counts");
    if (n1 > 0) c->hip(hipMemcpyAsync(counts, d_counts.p, (size_t)n1 * 8, hipMemcpyDeviceToHost, c->st), "d2h");
    c->hip(hipStreamSynchronize(c->st), "sync");
    return UMICLUST_OK;
  });
}

int32_t umiclust_overlap_regions(umiclust_ctx* ctx, const char* seqs, const int64_t* offs, int64_t n,
                                 const int64_t* region_start, int32_t nregions, int64_t* total, int32_t* maxcount) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (nregions < 1 || nregions > UMICLUST_OVERLAP_MAX_REGIONS || !total || !maxcount)
      c->fail(UMICLUST_EINVAL, "1..%d regions and both outputs required", UMICLUST_OVERLAP_MAX_REGIONS);
    OvRun R;
    overlap_table(c, R, seqs, offs, n, region_start, nregions, true);
    const size_t cells = (size_t)nregions * nregions;
    DevBuf<unsigned long long> d_total;
    DevBuf<uint32_t> d_max;
    c->hip(d_total.ensure(cells), "alloc");
    c->hip(d_max.ensure(cells), "alloc");
    c->hip(hipMemsetAsync(d_total.p, 0, cells * 8, c->st), "memset");
    c->hip(hipMemsetAsync(d_max.p, 0, cells * 4, c->st), "memset");
    if (n > 0) c->hip(launch_overlap_pairs(R.B, R.mask, nregions, d_total.p, d_max.p, c->st), "overlap pairs");
    std::vector<uint32_t> mx(cells);
    c->hip(hipMemcpyAsync(total, d_total.p, cells * 8, hipMemcpyDeviceToHost, c->st), "d2h");
    c->hip(hipMemcpyAsync(mx.data(), d_max.p, cells * 4, hipMemcpyDeviceToHost, c->st), "d2h");
    c->hip(hipStreamSynchronize(c->st), "sync");
    for (size_t x = 0; x < cells; x++) maxcount[x] = (int32_t)mx[x];
    return UMICLUST_OK;
  });
}
