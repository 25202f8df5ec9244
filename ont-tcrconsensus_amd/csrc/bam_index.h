// bam_index.h -- the .bai index and flagstat of a BAM stream, HIP-free (policies O10 and O11: restated
// from the SAM specification §5 and samtools' flagstat, not pinned to a samtools binary).
//
// The per-record rules are here once, for the host and for the device, on the layout of bam_record.h: what a record
// spans on its reference, its bin, the virtual offset of a stream position under a block table, the order and range
// tests, and which of the 32 flagstat counters it adds to.  bamindex.hip runs them one thread a record;
// bai::build_host below is the plain serial restatement of those kernels (tools/bai_check_main.cpp,
// tests/test_bai_cpu.py).  What follows the kernels -- the finish over the runs, the file's bytes, the flagstat text --
// is host code only and shared by both.
//
// The block table of a compressed file: block b starts at compressed offset coff[b] and holds the stream bytes
// [ustart[b], ustart[b + 1]); every block of the file is listed, empty ones too, and the last entry is the block that
// follows the data (the EOF block, or the file's end where there is none): ustart[nblocks - 1] = the stream's length.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "bam_record.h"  // the record's layout, and UC_HD

namespace uc {
namespace bai {

enum : int32_t { kOk = 0, kUnsorted = 1, kRange = 2, kBadRef = 3 };
constexpr int64_t kMaxEnd = (int64_t)1 << 29;  // what min_shift 14 and depth 5 address
constexpr int32_t kMetaBin = 37450;
constexpr int kCounters = 32;
// counter 2 * k + w: row k of the flagstat text, w = 1 for a QC-failed record
enum : int {
  kTotal = 0, kPrimary, kSecondary, kSupplementary, kDup, kPrimaryDup, kMapped, kPrimaryMapped, kPaired, kRead1,
  kRead2, kProper, kBothMapped, kSingleton, kDiffChr, kDiffChrQ5
};

// What the rules read of one record; rec = its block_size field.  The CIGAR is read inside the record only: a record
// whose fields overrun it (the session's open has named those among the primary ones) is cut there, never read past.
struct Rec {
  int32_t tid, next_tid;
  int64_t beg, end;
  uint32_t flag, mapq;
};
UC_HD inline Rec read_record(const uint8_t* rec) {
  Rec r;
  const int64_t bs = (int64_t)bam::block_size(rec);
  r.tid = bam::ref_id(rec);
  r.beg = bam::pos(rec);
  const int64_t lrn = bam::l_read_name(rec);
  r.mapq = bam::mapq(rec);
  int64_t ncig = bam::n_cigar_op(rec);
  r.flag = bam::flag(rec);
  r.next_tid = bam::next_ref_id(rec);
  ncig = ncig < (bs - 32 - lrn) / 4 ? ncig : (bs - 32 - lrn) / 4;
  int64_t rlen = 0;
  if (!(r.flag & bam::kFlagUnmapped) && ncig > 0) {
    const uint8_t* c = bam::cigar(rec, (uint32_t)lrn);
    for (int64_t k = 0; k < ncig; k++) {
      const uint32_t v = bam::le32(c + 4 * k);
      if (bam::op_on_reference(v & 15)) rlen += v >> 4;
    }
  }
  r.end = r.beg + bam::reference_span(rlen);
  return r;
}

// the record's own status: BAI cannot address it, or the header has no such reference
UC_HD inline int32_t range_status(const Rec& r, int32_t nref) {
  if (r.tid < 0) return kOk;
  if (r.tid >= nref) return kBadRef;
  return (r.beg < 0 || r.end > kMaxEnd) ? kRange : kOk;
}
// the order test against the kept record before it
UC_HD inline bool out_of_order(int32_t ptid, int64_t pbeg, int32_t tid, int64_t beg) {
  if ((uint32_t)tid < (uint32_t)ptid) return true;
  return tid == ptid && tid >= 0 && beg < pbeg;
}

// the virtual offset of stream position p, 0 < p <= ustart[nblocks - 1]: htslib's bgzf_tell after reading up to p
UC_HD inline uint64_t voffset(int64_t p, const int64_t* coff, const int64_t* ustart, int64_t nblocks) {
  int64_t lo = 0, hi = nblocks - 1;  // the last block b with ustart[b] <= p - 1: the one that holds byte p - 1
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ustart[mid] <= p - 1) lo = mid;
    else hi = mid - 1;
  }
  if (lo + 1 >= nblocks || p < ustart[lo + 1]) return ((uint64_t)coff[lo] << 16) | (uint64_t)(p - ustart[lo]);
  return (uint64_t)coff[lo + 1] << 16;
}

// bit k of the result: the record adds to row k of flagstat (its column is the QC-fail bit)
UC_HD inline uint32_t flagstat_rows(const Rec& r) {
  const uint32_t f = r.flag;
  uint32_t m = 1u << kTotal;
  if (f & bam::kFlagSecondary) m |= 1u << kSecondary;
  else if (f & bam::kFlagSupplementary) m |= 1u << kSupplementary;
  else {
    m |= 1u << kPrimary;
    if (f & 0x1) {
      m |= 1u << kPaired;
      if ((f & 0x2) && !(f & bam::kFlagUnmapped)) m |= 1u << kProper;
      if (f & 0x40) m |= 1u << kRead1;
      if (f & 0x80) m |= 1u << kRead2;
      if ((f & 0x8) && !(f & bam::kFlagUnmapped)) m |= 1u << kSingleton;
      if (!(f & bam::kFlagUnmapped) && !(f & 0x8)) {
        m |= 1u << kBothMapped;
        if (r.next_tid != r.tid) {
          m |= 1u << kDiffChr;
          if (r.mapq >= 5) m |= 1u << kDiffChrQ5;
        }
      }
    }
    if (!(f & bam::kFlagUnmapped)) m |= 1u << kPrimaryMapped;
    if (f & 0x400) m |= 1u << kPrimaryDup;
  }
  if (!(f & bam::kFlagUnmapped)) m |= 1u << kMapped;
  if (f & 0x400) m |= 1u << kDup;
  return m;
}

// ---------------------------------------------------------------- host only from here
// One run: consecutive kept records of one reference in one bin, from the first one's start to the last one's end.
struct Run {
  int32_t tid, bin;
  uint64_t u, v;
};
inline bool operator==(const Run& a, const Run& b) { return a.tid == b.tid && a.bin == b.bin && a.u == b.u && a.v == b.v; }

// What the kernels (or build_host) hand the finish: everything per kept record, per run and per reference.
struct Keys {
  int64_t nkept = 0, n_no_coor = 0;
  int64_t first_bad = -1;  // the first kept record (its index among all records) with a status
  int32_t first_status = kOk;
  std::vector<int32_t> tid, bin, w0, w1, status;  // per kept record (bin, w0, w1: 0 where tid < 0)
  std::vector<uint64_t> u, v;
  std::vector<Run> runs, sorted;           // in file order; stably sorted by (tid, bin)
  std::vector<int64_t> n_intv, base;       // per reference; base[nref] = all windows
  std::vector<uint64_t> linear;            // base[t] + w
  std::vector<int64_t> mapped, unmapped;   // per reference
  int64_t counters[kCounters] = {0};
};

// The host restatement of bamindex.hip: the same arrays from the same per-record functions, serially.  keep may be
// null (every record).  Without a block table (nblocks = 0) only the counters, the per-reference counts and the
// statuses are computed, as umiclust_bam_flagstat needs them.
inline void build_host(const uint8_t* raw, int64_t header_end, const std::vector<int64_t>& roff, const uint8_t* keep,
                       int32_t nref, const int64_t* coff, const int64_t* ustart, int64_t nblocks, Keys& K) {
  K = Keys();
  K.n_intv.assign((size_t)nref, 0), K.mapped.assign((size_t)nref, 0), K.unmapped.assign((size_t)nref, 0);
  int64_t pos = header_end, pbeg = 0;
  int32_t ptid = 0;
  bool have_prev = false;
  for (size_t r = 0; r < roff.size(); r++) {
    if (keep && !keep[r]) continue;
    const uint8_t* p = raw + roff[r];
    const Rec R = read_record(p);
    const int64_t size = 4 + (int64_t)bam::block_size(p);
    int32_t st = range_status(R, nref);
    if (!st && have_prev && out_of_order(ptid, pbeg, R.tid, R.beg)) st = kUnsorted;
    if (st && K.first_bad < 0) K.first_bad = (int64_t)r, K.first_status = st;
    const bool placed = R.tid >= 0 && R.tid < nref;
    const bool ok = placed && st != kRange;
    K.tid.push_back(R.tid), K.status.push_back(st);
    K.bin.push_back(ok ? bam::reg2bin(R.beg, R.end) : 0);
    K.w0.push_back(ok ? (int32_t)(R.beg >> 14) : 0), K.w1.push_back(ok ? (int32_t)((R.end - 1) >> 14) : 0);
    K.u.push_back(nblocks ? voffset(pos, coff, ustart, nblocks) : 0);
    K.v.push_back(nblocks ? voffset(pos + size, coff, ustart, nblocks) : 0);
    const uint32_t rows = flagstat_rows(R);
    for (int k = 0; k < 16; k++)
      if (rows >> k & 1) K.counters[2 * k + ((R.flag & bam::kFlagQcFail) ? 1 : 0)]++;
    if (R.tid < 0) K.n_no_coor++;
    if (placed) {
      ((R.flag & bam::kFlagUnmapped) ? K.unmapped : K.mapped)[(size_t)R.tid]++;
      if (ok) K.n_intv[(size_t)R.tid] = std::max<int64_t>(K.n_intv[(size_t)R.tid], K.w1.back() + 1);
    }
    pos += size, ptid = R.tid, pbeg = R.beg, have_prev = true;
  }
  K.nkept = (int64_t)K.tid.size();
  K.base.assign((size_t)nref + 1, 0);
  for (int32_t t = 0; t < nref; t++) K.base[(size_t)t + 1] = K.base[(size_t)t] + K.n_intv[(size_t)t];
  if (!nblocks || K.first_bad >= 0) return;
  for (int64_t j = 0; j < K.nkept; j++) {
    if (K.tid[j] < 0) continue;
    if (j == 0 || K.tid[j] != K.tid[j - 1] || K.bin[j] != K.bin[j - 1]) K.runs.push_back({K.tid[j], K.bin[j], K.u[j], K.v[j]});
    else K.runs.back().v = K.v[j];
  }
  K.sorted = K.runs;
  std::stable_sort(K.sorted.begin(), K.sorted.end(),
                   [](const Run& a, const Run& b) { return a.tid != b.tid ? a.tid < b.tid : a.bin < b.bin; });
  K.linear.assign((size_t)K.base[(size_t)nref], ~0ull);
  for (int64_t j = 0; j < K.nkept; j++)
    if (K.tid[j] >= 0)
      for (int64_t w = K.w0[j]; w <= K.w1[j]; w++) {
        uint64_t& x = K.linear[(size_t)(K.base[(size_t)K.tid[j]] + w)];
        x = std::min(x, K.u[j]);
      }
  for (int32_t t = 0; t < nref; t++)
    for (int64_t w = K.n_intv[(size_t)t] - 2; w >= 0; w--) {
      uint64_t* x = &K.linear[(size_t)(K.base[(size_t)t] + w)];
      if (x[0] == ~0ull) x[0] = x[1];
    }
}

typedef std::pair<uint64_t, uint64_t> Chunk;
// The finish of one reference over its runs [r0, r1) of `sorted`: small bins move up level by level, then neighbours
// in a bin merge.  Returns the bins in ascending number.
inline std::map<int32_t, std::vector<Chunk>> finish_ref(const std::vector<Run>& sorted, size_t r0, size_t r1) {
  std::map<int32_t, std::vector<Chunk>> bins;
  const auto by_start = [](const Chunk& a, const Chunk& b) { return a.first < b.first; };
  for (size_t r = r0; r < r1; r++) bins[sorted[r].bin].emplace_back(sorted[r].u, sorted[r].v);
  for (int L = 5; L >= 1; L--) {
    const int32_t lo = ((1 << 3 * L) - 1) / 7, hi = ((1 << 3 * (L + 1)) - 1) / 7;
    std::vector<int32_t> level;
    for (auto it = bins.lower_bound(lo); it != bins.end() && it->first < hi; ++it) level.push_back(it->first);
    for (int32_t b : level) {
      std::vector<Chunk>& c = bins[b];
      std::stable_sort(c.begin(), c.end(), by_start);
      if ((int64_t)(c.back().second >> 16) - (int64_t)(c.front().first >> 16) >= 0x10000) continue;
      std::vector<Chunk>& up = bins[(b - 1) >> 3];
      up.insert(up.end(), c.begin(), c.end());
      bins.erase(b);
    }
  }
  for (auto& kv : bins) {
    std::vector<Chunk>& c = kv.second;
    std::stable_sort(c.begin(), c.end(), by_start);
    size_t n = 0;
    for (size_t k = 1; k < c.size(); k++) {
      if ((c[n].second >> 16) >= (c[k].first >> 16)) c[n].second = std::max(c[n].second, c[k].second);
      else c[++n] = c[k];
    }
    c.resize(n + 1);
  }
  return bins;
}

// the file's bytes (SAM specification §5.2); *chunks (may be null): the chunks left after the finish
inline std::vector<uint8_t> serialise(const Keys& K, int32_t nref, int64_t* chunks = nullptr) {
  std::vector<uint8_t> out;
  const auto p32 = [&](uint32_t v) {
    for (int k = 0; k < 4; k++) out.push_back((uint8_t)(v >> (8 * k)));
  };
  const auto p64 = [&](uint64_t v) {
    for (int k = 0; k < 8; k++) out.push_back((uint8_t)(v >> (8 * k)));
  };
  out.insert(out.end(), {'B', 'A', 'I', 1});
  p32((uint32_t)nref);
  size_t r = 0;
  int64_t nchunks = 0;
  for (int32_t t = 0; t < nref; t++) {
    const size_t r0 = r;
    while (r < K.sorted.size() && K.sorted[r].tid == t) r++;
    if (K.mapped[(size_t)t] + K.unmapped[(size_t)t] == 0) {
      p32(0), p32(0);
      continue;
    }
    const auto bins = finish_ref(K.sorted, r0, r);
    uint64_t first = ~0ull, last = 0;
    for (size_t x = r0; x < r; x++) first = std::min(first, K.sorted[x].u), last = std::max(last, K.sorted[x].v);
    p32((uint32_t)bins.size() + 1);
    for (const auto& kv : bins) {
      p32((uint32_t)kv.first), p32((uint32_t)kv.second.size());
      for (const Chunk& c : kv.second) p64(c.first), p64(c.second);
      nchunks += (int64_t)kv.second.size();
    }
    p32((uint32_t)kMetaBin), p32(2), p64(first), p64(last), p64((uint64_t)K.mapped[(size_t)t]), p64((uint64_t)K.unmapped[(size_t)t]);
    p32((uint32_t)K.n_intv[(size_t)t]);
    for (int64_t w = 0; w < K.n_intv[(size_t)t]; w++) p64(K.linear[(size_t)(K.base[(size_t)t] + w)]);
  }
  p64((uint64_t)K.n_no_coor);
  if (chunks) *chunks = nchunks;
  return out;
}

// ---- O11: the text of samtools >= 1.13 over the 32 counters
inline std::string flagstat_text(const int64_t* c) {
  static const char* const label[16] = {
      "in total (QC-passed reads + QC-failed reads)", "primary", "secondary", "supplementary", "duplicates",
      "primary duplicates", "mapped", "primary mapped", "paired in sequencing", "read1", "read2", "properly paired",
      "with itself and mate mapped", "singletons", "with mate mapped to a different chr",
      "with mate mapped to a different chr (mapQ>=5)"};
  const auto pct = [](int64_t n, int64_t total) {
    char b[32];
    if (total) snprintf(b, sizeof b, "%.2f%%", (float)n / (float)total * 100.0);
    else snprintf(b, sizeof b, "N/A");
    return std::string(b);
  };
  std::string out;
  for (int k = 0; k < 16; k++) {
    char b[160];
    snprintf(b, sizeof b, "%lld + %lld %s", (long long)c[2 * k], (long long)c[2 * k + 1], label[k]);
    out += b;
    const int den = k == kMapped ? kTotal : k == kPrimaryMapped ? kPrimary : (k == kProper || k == kSingleton) ? kPaired : -1;
    if (den >= 0) out += " (" + pct(c[2 * k], c[2 * den]) + " : " + pct(c[2 * k + 1], c[2 * den + 1]) + ")";
    out += "\n";
  }
  return out;
}

}  // namespace bai
}  // namespace uc
