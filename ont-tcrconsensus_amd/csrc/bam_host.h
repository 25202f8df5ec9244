// bam_host.h -- the HIP-free host side of the BAM readers and of the BAM writer (rows f4 and f6):
// header parsing and record offsets (shared by umiclust_region_split and the umiclust_bam_* session), the serial walk
// of k_bam_scan (csrc/bamscan.hip) over the rules of bam_record.h, and the BGZF writer.  Compiled by g++ (no HIP), so the CPU suite
// builds it with ASan + UBSan (tools/bam_check_main.cpp, tests/test_bam_filter_cpu.py).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bam_record.h"

namespace uc {
namespace bam {

struct Header {
  size_t text_len = 0;                 // l_text
  std::vector<std::string> ref_name;   // without the NUL
  std::vector<int64_t> ref_len;
  size_t end = 0;                      // offset of the first record = the bytes a writer copies verbatim
};
// raw = the inflated file.  false + err: not BAM / a header field runs past the buffer
bool parse_header(const uint8_t* raw, size_t n, Header& h, std::string& err);
// offsets of every record's block_size field from `start` on; false + err when the last record is cut short or a
// block_size is smaller than the 32 fixed bytes
bool record_offsets(const uint8_t* raw, size_t n, size_t start, std::vector<int64_t>& roff, std::string& err);

// the variable-length fields of every record stay inside the record (bam::fits).  The f4 kernels (regionsplit.hip)
// index the name, the CIGAR and the sequence by these fields alone, so umiclust_region_split checks them before any
// launch.  false + err naming the first record that fails
bool check_record_fields(const uint8_t* raw, const std::vector<int64_t>& roff, std::string& err);

// ---- the per-record columns of k_bam_scan (the cs hash: bam_record.h) ----
enum : int8_t { kScanUnmapped = 0, kScanSecondary = 1, kScanPrimary = 2 };
struct ScanRow {
  int8_t cls = 0, bad = 0;
  uint8_t nm_present = 0;
  int32_t ref = -1, l_seq = 0, cs_len = -1;
  int64_t reference_length = 0, cols = 0, nm = 0, cs_off = 0;
  uint64_t cs_hash = 0;
};
// one record, exactly as the kernel computes it (roff = offset of its block_size field)
void scan_record(const uint8_t* raw, int64_t roff, uint64_t seed, uint64_t hmask, ScanRow& out);

// ---- the detected-UMI record of one BAM record (row f4+f1) ----
// The read as k_bam_emit (regionsplit.hip) writes it: the forward sequence (bam::forward_base), "None" for a record
// without one.  rec = the record's block_size field; its fields have been checked.
std::string forward_text(const uint8_t* rec);
// What extract_umis.py prints for the FASTA entry ">{name};strand={+|-}" + forward_text, given the six values of
// umiclust_extract_umis (both UMIs found) and the 3' window length a3: read name = header up to its first ';', strand
// = header.split("strand=")[1], combined UMI = u5 + u3 on "+", their reverse complements swapped on anything else.
// The serial counterpart of k_bam_emit_umi, and the formatter of the records whose name holds "strand=".
std::string format_umi_record(const uint8_t* rec, const int32_t* res, int32_t a3);

// ---- BGZF writer ----
// The file at `path` inflates to raw[0, header_end) followed by the records r with keep[r] != 0 (record r =
// raw[roff[r], roff[r] + 4 + block_size)), in input order: blocks of at most 0xff00 payload bytes, raw deflate, the BC
// extra field with BSIZE, CRC32 and ISIZE, then the 28-byte EOF block.  Blocks are compressed on `threads` threads
// and written in order.  Returns the number of records written, -1 + err on an I/O failure.  coff (may be null): the
// compressed offset of every block written, the EOF block's last.
int64_t write_bgzf(const char* path, const uint8_t* raw, size_t header_end, const std::vector<int64_t>& roff,
                   const uint8_t* keep, int threads, std::string& err, std::vector<int64_t>* coff = nullptr);

// The pieces of it that the device writer (dropin_bgzf.cpp) shares.
constexpr size_t kBgzfPayload = 0xff00;
extern const uint8_t kBgzfEof[28];
// The uncompressed stream as segments of raw: the header bytes, then the kept records (a run of adjacent kept records
// is one segment); seg_at[k] = stream offset of segment k.  Blocks are cut from the segments directly, so the stream
// itself is never materialised.
struct BgzfStream {
  const uint8_t* raw = nullptr;
  std::vector<std::pair<size_t, size_t>> seg;  // (offset in raw, length)
  std::vector<size_t> seg_at;
  size_t total = 0;
  int64_t nkept = 0;
  size_t blocks() const { return (total + kBgzfPayload - 1) / kBgzfPayload; }
  size_t block_bytes(size_t b) const { return std::min(kBgzfPayload, total - b * kBgzfPayload); }
  void gather(size_t at, size_t n, uint8_t* dst) const;  // stream bytes [at, at + n) to dst
};
BgzfStream bgzf_stream(const uint8_t* raw, size_t header_end, const std::vector<int64_t>& roff, const uint8_t* keep);
// blocks [b0, b1) of the stream to dst (block b at (b - b0) * 0xff00) and the CRC32 of each to crc[b - b0], on
// `threads` threads
void bgzf_gather_crc(const BgzfStream& S, size_t b0, size_t b1, uint8_t* dst, uint32_t* crc, int threads);
// one block of at most 0xff00 bytes by zlib at level 6, framed (level 0 if the deflated form would not fit BSIZE)
bool bgzf_block(const uint8_t* src, size_t n, std::vector<uint8_t>& out);
bool write_fd(int fd, const uint8_t* p, size_t n);
uint32_t bgzf_crc32(const uint8_t* p, size_t n);  // zlib's

}  // namespace bam
}  // namespace uc
