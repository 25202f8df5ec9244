// bai_check_main.cpp -- drives the HIP-free side of the .bai index and flagstat (ont-tcrconsensus_amd/csrc/bam_index.h)
// under ASan + UBSan, without a GPU (make bai_check; tests/test_bai_cpu.py).  The device is replaced by
// bai::build_host, the host restatement of the kernels of bamindex.hip; the finish, the file's bytes and the flagstat
// text are the code the library runs.
//
//   bai_check file <in.bam> <out.bai> <out.flagstat>
//       the index of a BGZF file: the block table from io::bgzf_blocks, the stream from io::inflate_bgzf
//   bai_check case <in.case> <out.bai> <out.flagstat>
//       the index of a stream under a block table the case gives: three int64 (stream bytes, keep bytes or -1 for
//       every record, blocks), the stream, the keep bytes, coff[blocks], ustart[blocks]
// Prints `ok kept=<n> runs=<n> chunks=<n> windows=<n>` and writes both files, or prints
// `refused status=<1 unsorted | 2 range | 3 reference> record=<r>` and writes the flagstat alone.  Exit status 0, or
// 2 with `err=<message>` for input that is not BGZF / BAM / a case.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../ont-tcrconsensus_amd/csrc/bam_host.h"
#include "../ont-tcrconsensus_amd/csrc/bam_index.h"
#include "../ont-tcrconsensus_amd/csrc/host_io.h"

using namespace uc;

static bool slurp(const char* path, std::vector<uint8_t>& out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return true;
}
static bool spill(const char* path, const void* p, size_t n) {
  FILE* f = fopen(path, "wb");
  const bool ok = f && fwrite(p, 1, n, f) == n;
  return (!f || fclose(f) == 0) && ok;
}

int main(int argc, char** argv) {
  if (argc != 5 || (strcmp(argv[1], "file") && strcmp(argv[1], "case"))) {
    fprintf(stderr, "usage: bai_check file|case <in> <out.bai> <out.flagstat>\n");
    return 1;
  }
  std::vector<uint8_t> raw, keep;
  std::vector<int64_t> coff, ustart;
  bool have_keep = false;
  if (!strcmp(argv[1], "file")) {
    std::vector<uint8_t> file;
    std::vector<size_t> boff, bsz;
    std::vector<uint32_t> isz;
    if (!slurp(argv[2], file) || !io::bgzf_blocks(file.data(), file.size(), boff, bsz, isz) || !io::inflate_bgzf(argv[2], raw)) {
      printf("err=cannot read BGZF %s\n", argv[2]);
      return 2;
    }
    int64_t at = 0;
    for (size_t b = 0; b < boff.size(); b++) coff.push_back((int64_t)boff[b]), ustart.push_back(at), at += isz[b];
    if (isz.empty() || isz.back()) coff.push_back((int64_t)file.size()), ustart.push_back(at);
  } else {
    std::vector<uint8_t> in;
    int64_t h[3];
    if (!slurp(argv[2], in) || in.size() < sizeof h) {
      printf("err=cannot read %s\n", argv[2]);
      return 2;
    }
    memcpy(h, in.data(), sizeof h);
    const int64_t nkeep = h[1] < 0 ? 0 : h[1];
    if (h[0] < 0 || h[2] < 1 || in.size() != sizeof h + (size_t)h[0] + (size_t)nkeep + 16 * (size_t)h[2]) {
      printf("err=%s is no case\n", argv[2]);
      return 2;
    }
    const uint8_t* p = in.data() + sizeof h;
    raw.assign(p, p + h[0]), keep.assign(p + h[0], p + h[0] + nkeep);
    have_keep = h[1] >= 0;
    coff.resize((size_t)h[2]), ustart.resize((size_t)h[2]);
    memcpy(coff.data(), p + h[0] + nkeep, 8 * (size_t)h[2]);
    memcpy(ustart.data(), p + h[0] + nkeep + 8 * h[2], 8 * (size_t)h[2]);
  }
  bam::Header hdr;
  std::vector<int64_t> roff;
  std::string err;
  if (!bam::parse_header(raw.data(), raw.size(), hdr, err) || !bam::record_offsets(raw.data(), raw.size(), hdr.end, roff, err)) {
    printf("err=%s\n", err.c_str());
    return 2;
  }
  if (have_keep && keep.size() != roff.size()) {
    printf("err=%zu keep bytes for %zu records\n", keep.size(), roff.size());
    return 2;
  }
  const int32_t nref = (int32_t)hdr.ref_name.size();
  bai::Keys K;
  bai::build_host(raw.data(), (int64_t)hdr.end, roff, have_keep ? keep.data() : nullptr, nref, coff.data(), ustart.data(),
                  (int64_t)coff.size(), K);
  const std::string text = bai::flagstat_text(K.counters);
  if (!spill(argv[4], text.data(), text.size())) {
    printf("err=cannot write %s\n", argv[4]);
    return 2;
  }
  if (K.first_bad >= 0) {
    printf("refused status=%d record=%lld\n", K.first_status, (long long)K.first_bad);
    return 0;
  }
  int64_t chunks = 0;
  const std::vector<uint8_t> bytes = bai::serialise(K, nref, &chunks);
  if (!spill(argv[3], bytes.data(), bytes.size())) {
    printf("err=cannot write %s\n", argv[3]);
    return 2;
  }
  printf("ok kept=%lld runs=%zu chunks=%lld windows=%lld\n", (long long)K.nkept, K.sorted.size(), (long long)chunks,
         (long long)K.base.back());
  return 0;
}
