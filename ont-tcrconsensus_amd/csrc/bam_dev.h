// bam_dev.h -- what the five host files of the BAM drop-ins need of each other: dropin_bgzf.cpp (BGZF on the device),
// dropin_sam.cpp (SAM text to raw), dropin_split.cpp (the region split), dropin_bam.cpp (the session) and
// dropin_index.cpp (the .bai index and flagstat).  Declarations only.  (The radix sort that dropin_sam.cpp and
// dropin_index.cpp share is launch_sam_sort of umiclust_internal.h, which this header brings in through ctx.h.)
#pragma once
#include <string>
#include <string_view>
#include <vector>

#include "ctx.h"

namespace uc {

// ---- dropin_bgzf.cpp
// The bytes of `path`: a regular file is mapped; any other readable path (a FIFO, /dev/fd/N) is read to its end, or
// refused (regular_only).
struct InputBytes {
  void* map = nullptr;
  size_t map_n = 0;
  std::vector<uint8_t> buf;
  const uint8_t* p = nullptr;
  size_t n = 0;
  ~InputBytes();
  bool read(const char* path, bool regular_only);
};
// raw sized to `bytes` with its pages touched by the I/O threads
uint8_t* alloc_touched(RawBuf& raw, size_t bytes);
// What both BAM readers start with: the file inflated on the device into d_raw and copied back into `raw`.  info: BGZF
// blocks, blocks inflated on the device, compressed bytes uploaded; *t_upload (may be null): seconds of the upload.
// table (may be null): the file's block table as bam_index.h reads it.
struct BlockTable {
  std::vector<int64_t> coff, ustart;
};
bool read_bam_on_device(Ctx* c, const char* path, RawBuf& raw, DevBuf<uint8_t>& d_raw, int64_t info[3],
                        double* t_upload, BlockTable* table = nullptr);
// umiclust_bam_write on the device: the records written, -1 + err, or -2 for the caller to take the host writer
int64_t write_bgzf_device(Ctx* c, BamSession& S, const uint8_t* keep, const char* path, std::string& err);

// ---- dropin_sam.cpp
// the sibling of read_bam_on_device for SAM text; fails the context where that one returns false
void read_sam_on_device(Ctx* c, const char* path, RawBuf& raw, DevBuf<uint8_t>& d_raw, int64_t info[4],
                        double times[5]);

// ---- dropin_bam.cpp
// the open session, or UMICLUST_ESTATE
BamSession* bam_session(Ctx* c);
// the query name of record r: at most l_read_name bytes and never past the record, up to its NUL
std::string_view record_name(const RawBuf& raw, const std::vector<int64_t>& roff, int64_t r);
// The session holds the inflated file and its columns on the host only (ctx.h BamSession): a call that launches a
// kernel on it uploads the raw bytes and the record offsets with this and frees them on return.
void upload_session(Ctx* c, const BamSession& S, DevBuf<uint8_t>& d_raw, DevBuf<int64_t>& d_roff);

}  // namespace uc
