// bam_check_main.cpp -- drives the HIP-free side of the BAM session (ont-tcrconsensus_amd/csrc/bam_host.cpp) under
// ASan + UBSan, without a GPU (make bam_check; tests/test_bam_filter_cpu.py).  The device is replaced by
// bam::scan_record, the serial walk of k_bam_scan over the same rules (csrc/bam_record.h).
//
//   bam_check <in.bam> <out prefix> <threads>
//       inflates the file, parses the header, finds the record offsets, scans every record and prints
//         refs=<n> then one `ref <name> <length>` line per reference,
//         records=<n>, `fields=ok` or `fields=<message of bam::check_record_fields>` (what umiclust_region_split
//         refuses before its kernels run), then per record
//         `fix <r> refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen aux_offset`, the fixed
//         fields as the accessors of bam_record.h read them and bam::aux_offset of the three lengths, and
//         `rec <r> cls ref l_seq reference_length cols nm nm_present cs_len bad cs=<string>`,
//       then round-trips the writer twice -- every record kept (<prefix>.all.bam) and every second record kept
//       (<prefix>.alt.bam) -- re-inflates both and compares them with the header bytes + the kept records; prints
//       `roundtrip ok`.  Exit status 0, or 2 with `err=<message>` when the file is not BGZF / BAM.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../ont-tcrconsensus_amd/csrc/bam_host.h"
#include "../ont-tcrconsensus_amd/csrc/host_io.h"

using namespace uc;

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: bam_check <in.bam> <out prefix> <threads>\n");
    return 1;
  }
  const int threads = atoi(argv[3]);
  std::vector<uint8_t> raw;
  if (!io::inflate_bgzf(argv[1], raw)) {
    printf("err=cannot read BGZF %s\n", argv[1]);
    return 2;
  }
  bam::Header hdr;
  std::vector<int64_t> roff;
  std::string err;
  if (!bam::parse_header(raw.data(), raw.size(), hdr, err) ||
      !bam::record_offsets(raw.data(), raw.size(), hdr.end, roff, err)) {
    printf("err=%s\n", err.c_str());
    return 2;
  }
  printf("refs=%zu\n", hdr.ref_name.size());
  for (size_t r = 0; r < hdr.ref_name.size(); r++) printf("ref %s %lld\n", hdr.ref_name[r].c_str(), (long long)hdr.ref_len[r]);
  printf("records=%zu\n", roff.size());
  printf("fields=%s\n", bam::check_record_fields(raw.data(), roff, err) ? "ok" : err.c_str());
  for (size_t r = 0; r < roff.size(); r++) {
    const uint8_t* rec = raw.data() + roff[r];
    printf("fix %zu %d %d %u %u %u %u %u %d %d %d %d %lld\n", r, bam::ref_id(rec), bam::pos(rec), bam::l_read_name(rec),
           bam::mapq(rec), bam::bin(rec), bam::n_cigar_op(rec), bam::flag(rec), bam::l_seq(rec), bam::next_ref_id(rec),
           bam::next_pos(rec), bam::tlen(rec),
           (long long)bam::aux_offset(bam::l_read_name(rec), bam::n_cigar_op(rec), bam::l_seq(rec)));
    bam::ScanRow s;
    bam::scan_record(raw.data(), roff[r], bam::cs_seed(0), ~0ull, s);
    // the hash is a function of the bytes and the length alone, and never the table's empty key
    if (s.cs_len >= 0) {
      uint64_t sum = 0;
      for (int32_t x = 0; x < s.cs_len; x++) sum += bam::cs_term(bam::cs_seed(0), (uint64_t)x, raw[(size_t)s.cs_off + (size_t)x]);
      if (s.cs_hash != bam::cs_finish(sum, (uint64_t)s.cs_len, ~0ull) || s.cs_hash == bam::kCsEmpty || raw[(size_t)s.cs_off + (size_t)s.cs_len] != 0) {
        printf("err=record %zu: cs hash or span is wrong\n", r);
        return 3;
      }
    }
    printf("rec %zu %d %d %d %lld %lld %lld %d %d %d cs=%s\n", r, (int)s.cls, s.ref, s.l_seq, (long long)s.reference_length,
           (long long)s.cols, (long long)s.nm, (int)s.nm_present, s.cs_len, (int)s.bad,
           s.cs_len > 0 ? std::string((const char*)raw.data() + s.cs_off, (size_t)s.cs_len).c_str() : "");
  }
  for (int mode = 0; mode < 2; mode++) {
    std::vector<uint8_t> keep(roff.size() + 1, 0), want(raw.begin(), raw.begin() + (long)hdr.end), got;
    int64_t nkeep = 0;
    for (size_t r = 0; r < roff.size(); r++)
      if (mode == 0 || r % 2 == 0) {
        keep[r] = 1;
        nkeep++;
        const uint8_t* p = raw.data() + roff[r];
        want.insert(want.end(), p, p + 4 + bam::block_size(p));
      }
    const std::string path = std::string(argv[2]) + (mode == 0 ? ".all.bam" : ".alt.bam");
    const int64_t k = bam::write_bgzf(path.c_str(), raw.data(), hdr.end, roff, keep.data(), threads, err);
    if (k != nkeep) {
      printf("err=write_bgzf returned %lld, not %lld: %s\n", (long long)k, (long long)nkeep, err.c_str());
      return 3;
    }
    if (!io::inflate_bgzf(path.c_str(), got) || got != want) {
      printf("err=%s does not inflate to the header and the kept records\n", path.c_str());
      return 3;
    }
  }
  printf("roundtrip ok\n");
  return 0;
}
