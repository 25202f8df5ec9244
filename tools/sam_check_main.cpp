// sam_check_main.cpp -- stand-alone driver of the host restatement of csrc/sam_text.h, built with
// ASan + UBSan by tests/test_sam_text_cpu.py (make -C ont-tcrconsensus_amd sam_check).
//
//   sam_check CASES
// CASES holds SAM texts one after another, each as a little-endian uint32 byte count and the bytes.  For every case
// one line goes to stdout:
//   ok <records> <hex of raw> <roff, comma separated or ->
//   refused <EFORMAT|ERANGE> <message>
#include <cstdio>
#include <string>
#include <vector>

#include "../ont-tcrconsensus_amd/csrc/sam_text.h"

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: sam_check CASES\n"), 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  std::vector<uint8_t> all;
  uint8_t buf[1 << 16];
  for (size_t k; (k = fread(buf, 1, sizeof(buf), fh)) > 0;) all.insert(all.end(), buf, buf + k);
  fclose(fh);
  for (size_t o = 0; o < all.size();) {
    if (o + 4 > all.size()) return fprintf(stderr, "truncated case file\n"), 2;
    const size_t n = (size_t)all[o] | ((size_t)all[o + 1] << 8) | ((size_t)all[o + 2] << 16) | ((size_t)all[o + 3] << 24);
    o += 4;
    if (o + n > all.size()) return fprintf(stderr, "truncated case file\n"), 2;
    // a copy of exactly n bytes, so that a read past the text is a read past an allocation
    const std::vector<uint8_t> text(all.begin() + (long)o, all.begin() + (long)(o + n));
    o += n;
    std::vector<uint8_t> raw;
    std::vector<int64_t> roff;
    std::string err;
    const int32_t rc = uc::sam::encode_host(text.data(), text.size(), raw, roff, err);
    if (rc != uc::sam::kOk) {
      printf("refused %s %s\n", rc == uc::sam::kERange ? "ERANGE" : "EFORMAT", err.c_str());
      continue;
    }
    std::string hex;
    static const char* const digits = "0123456789abcdef";
    for (uint8_t b : raw) hex += digits[b >> 4], hex += digits[b & 15];
    printf("ok %zu %s ", roff.size(), hex.c_str());
    if (roff.empty()) printf("-");
    for (size_t r = 0; r < roff.size(); r++) printf("%s%lld", r ? "," : "", (long long)roff[r]);
    printf("\n");
  }
  return 0;
}
