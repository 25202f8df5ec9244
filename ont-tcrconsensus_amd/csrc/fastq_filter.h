// fastq_filter.h -- the HIP-free host side of the `vsearch --fastq_filter` drop-in (row f5): the
// argv grammar, the streaming record indexer over the mapped input, the keep/discard decision (policy O7d) with its
// guard band and host recheck, and the in-order writers.  The per-record fixed-point expected-error sums come from
// a Backend: the device (dropin_fastq.cpp, csrc/fastq_filter.hip) or the host restatement below
// (tools/fastq_check_main.cpp, the CPU suite's ASan/UBSan program).  Compiled by g++ (no HIP); depends on no other
// translation unit.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/umiclust.h"

namespace uc {
namespace fq {

constexpr int kFxShift = 40;                 // ee_fx = sum of llrint(p[q] * 2^40)
constexpr int64_t kDevMaxLen = 1ll << 22;    // longer records could overflow the int64 sum: evaluated on the host
constexpr int64_t kPad = 16;                 // bytes before and after the concatenated qualities (16-byte lane loads)
constexpr int64_t kChunkDefault = 64ll << 20;  // quality bytes per chunk (UMICLUST_FQ_CHUNK)
constexpr int64_t kChunkMin = 1024;

// p[b] = pow(10, -(b - ascii) / 10) and fx[b] = llrint(ldexp(p[b], 40)) for raw bytes b with qmin <= b - ascii <= qmax,
// 0 elsewhere; [lo, hi] = the raw bytes in range
struct Tables {
  uint64_t fx[256];
  double p[256];
  int lo = 0, hi = 0;
};
void build_tables(int ascii, int qmin, int qmax, Tables& t);

// One record of the input.  Offsets point into the mapping, or into the chunk's arena for a record whose sequence or
// quality spans several lines (joined there).
struct Rec {
  int64_t begin = 0, end = 0;  // the record's bytes in the mapping, [begin, end)
  int64_t label = 0;           // label start (after '@'), in the mapping
  int64_t seq = 0, qual = 0;   // len bytes each
  int64_t len = 0;
  int32_t label_len = 0;       // header truncated at the first space or tab
  uint8_t arena = 0;           // seq / qual are arena offsets
  uint8_t verbatim = 0;        // [begin, end) is already `@label\nSEQ\n+\nQUAL\n`
};

// Index the records that start in [pos, want_end) of a mapped FASTQ on T threads (slices resynchronised on the
// 4-line shape and checked against each other at the seams); *next = the first byte after the last record indexed.
// A file that is not 4-line FASTQ sets *multi_line and is indexed by one sequential indexer from then on.  Returns
// UMICLUST_OK, or UMICLUST_EFORMAT with recs holding the records before the malformed one.
int index_window(const char* data, int64_t size, int64_t pos, int64_t want_end, int T, std::vector<Rec>& recs,
                 std::vector<char>& arena, int64_t* next, bool* multi_line, std::string& err);

// A chunk's staging arrays (host-visible): qual = kPad zero bytes, the gathered qualities, kPad zero bytes;
// offs[n + 1] relative to qual + kPad; the outputs per record
struct Slot {
  uint8_t* qual = nullptr;
  int64_t* offs = nullptr;
  int64_t* ee = nullptr;
  uint8_t* qlo = nullptr;
  uint8_t* qhi = nullptr;
};

// Where the per-record sums are computed.  reserve() is called from the parsing thread, run() from the caller's.
struct Backend {
  virtual ~Backend() = default;
  virtual bool reserve(int slot, size_t qual_bytes, size_t nrec, Slot& s, std::string& err) = 0;
  // ee[i] = sum of table[b], qlo[i] / qhi[i] = min / max of b over record i's bytes (255 / 0 for an empty record)
  virtual bool run(int slot, size_t qual_bytes, int64_t nrec, const uint64_t* table, double* t_h2d_s,
                   double* t_kernel_s, std::string& err) = 0;
};

// the host restatement of the kernel
struct HostBackend : Backend {
  std::vector<uint8_t> q[2], lo[2], hi[2];
  std::vector<int64_t> offs[2], ee[2];
  Slot slots[2];
  bool reserve(int slot, size_t qual_bytes, size_t nrec, Slot& s, std::string& err) override;
  bool run(int slot, size_t qual_bytes, int64_t nrec, const uint64_t* table, double* t_h2d_s, double* t_kernel_s,
           std::string& err) override;
};

// O7c / O7d exactly: 0 kept, 1 short, 2 long, 3 maxee, 4 maxee_rate
int decide_exact(const umiclust_fastq_filter_params& p, const Tables& t, const uint8_t* qual, int64_t len);
// The same decision from the fixed-point sum; *in_band = 1 (and nothing decided, returns -1) when ee_fx * 2^-40 lies
// within the guard band of a threshold that is given
int decide_fx(const umiclust_fastq_filter_params& p, int64_t len, int64_t ee_fx, int* in_band);

struct Paths {
  const char* in = nullptr;
  const char* out = nullptr;        // may be null
  const char* discarded = nullptr;  // may be null
  const char* log = nullptr;        // may be null
};

// The whole step.  Returns n_kept or a negative UMICLUST_E* code with err set.
int64_t run_filter(const umiclust_fastq_filter_params& p, const Paths& paths, int threads, int64_t chunk_bytes,
                   Backend& be, umiclust_fastq_filter_result* res, std::string& err);

}  // namespace fq
}  // namespace uc
