// umi_text_check_main.cpp -- drives the HIP-free formatter of the fused split + extract (row f4+f1, DESIGN.md §9d:
// bam::forward_text and bam::format_umi_record in ont-tcrconsensus_amd/csrc/bam_host.cpp) under ASan + UBSan, without
// a GPU (make umi_text_check; tests/test_split_extract_cpu.py).
//
//   umi_text_check <in.bam> <results> <a3> <out>
//       <results> holds six integers per record of the BAM (umiclust_extract_umis' values; the test computes them with
//       oracle/extract.py).  Writes to <out> the forward text of every record, one per line, then a line `--`, then
//       the detected-UMI text of every record whose two distances are >= 0.  Exit status 0, or 2 with a message.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../ont-tcrconsensus_amd/csrc/bam_host.h"
#include "../ont-tcrconsensus_amd/csrc/host_io.h"

using namespace uc;

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: umi_text_check <in.bam> <results> <a3> <out>\n");
    return 1;
  }
  std::vector<uint8_t> raw;
  bam::Header hdr;
  std::vector<int64_t> roff;
  std::string err;
  if (!io::inflate_bgzf(argv[1], raw) || !bam::parse_header(raw.data(), raw.size(), hdr, err) ||
      !bam::record_offsets(raw.data(), raw.size(), hdr.end, roff, err) ||
      !bam::check_record_fields(raw.data(), roff, err)) {
    fprintf(stderr, "cannot read %s: %s\n", argv[1], err.c_str());
    return 2;
  }
  std::vector<int32_t> res(roff.size() * 6);
  FILE* fr = fopen(argv[2], "r");
  if (!fr) return 2;
  for (int32_t& v : res)
    if (fscanf(fr, "%d", &v) != 1) {
      fprintf(stderr, "too few results\n");
      fclose(fr);
      return 2;
    }
  fclose(fr);
  const int32_t a3 = atoi(argv[3]);
  FILE* fo = fopen(argv[4], "wb");
  if (!fo) return 2;
  for (size_t r = 0; r < roff.size(); r++) fprintf(fo, "%s\n", bam::forward_text(raw.data() + roff[r]).c_str());
  fprintf(fo, "--\n");
  for (size_t r = 0; r < roff.size(); r++) {
    const int32_t* q = res.data() + r * 6;
    if (q[0] < 0 || q[3] < 0) continue;
    const std::string t = bam::format_umi_record(raw.data() + roff[r], q, a3);
    fwrite(t.data(), 1, t.size(), fo);
  }
  return fclose(fo) == 0 ? 0 : 2;
}
