// inflate_check_main.cpp -- drives the HIP-free DEFLATE decoder (ont-tcrconsensus_amd/csrc/inflate.h) and the BGZF
// framing walk (io::bgzf_blocks of host_io.cpp) under ASan + UBSan, without a GPU (make inflate_check;
// tests/test_bgzf_inflate_cpu.py; tests/test_gpu_bgzf_inflate.py builds it without the sanitizers as its pre-check).
// uc::inflate_block is the host restatement of k_bgzf_inflate.
//
//   inflate_check cases <file>
//       <file> = u32 count, then per block `u32 payload bytes, u32 ISIZE, u32 accepted`, the payload, and the ISIZE
//       expected bytes where accepted (tests/inflate_cases.py write_case_file).  Every payload and every output gets a
//       heap block of exactly its size, so a byte read or written past either is a sanitizer report.  Per block the
//       decoder must accept exactly when the file says so and when zlib does under the host reader's rule
//       (Z_STREAM_END with avail_out == 0), and give the expected bytes.  Prints `bad <i> ...` per difference, then
//       `blocks=<n> accepted=<a> rejected=<r> bad=<b>` and one `class <k> <count>` line per status; exit 0 iff bad=0.
//   inflate_check frames <file>
//       prints `frames ok <blocks> <sum of ISIZE>` or `frames bad`
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../ont-tcrconsensus_amd/csrc/host_io.h"
#include "../ont-tcrconsensus_amd/csrc/inflate.h"

namespace {
bool read_file(const char* path, std::vector<uint8_t>& d) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  d.resize((size_t)n);
  const bool ok = n == 0 || fread(d.data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  return ok;
}
uint32_t u32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
// the host reader's rule (io::inflate_bgzf)
bool zlib_accepts(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t isize) {
  z_stream zs{};
  if (inflateInit2(&zs, -15) != Z_OK) return false;
  zs.next_in = const_cast<Bytef*>(in);
  zs.avail_in = n;
  zs.next_out = out;
  zs.avail_out = isize;
  const int rc = inflate(&zs, Z_FINISH);
  inflateEnd(&zs);
  return rc == Z_STREAM_END && zs.avail_out == 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: inflate_check cases|frames <file>\n");
    return 1;
  }
  std::vector<uint8_t> d;
  if (!read_file(argv[2], d)) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 1;
  }
  if (!strcmp(argv[1], "frames")) {
    std::vector<size_t> boff, bsz;
    std::vector<uint32_t> isz;
    // a heap block of exactly the file's size: a read past it is a report
    std::unique_ptr<uint8_t[]> f(new uint8_t[d.size()]);
    if (!d.empty()) memcpy(f.get(), d.data(), d.size());
    if (!uc::io::bgzf_blocks(f.get(), d.size(), boff, bsz, isz)) {
      printf("frames bad\n");
      return 0;
    }
    unsigned long long sum = 0;
    for (uint32_t v : isz) sum += v;
    printf("frames ok %zu %llu\n", boff.size(), sum);
    return 0;
  }
  if (strcmp(argv[1], "cases") || d.size() < 4) return 1;
  const uint32_t n = u32(d.data());
  size_t o = 4;
  long accepted = 0, bad = 0, cls[uc::inf::kNumStatus] = {};
  for (uint32_t i = 0; i < n; i++) {
    if (o + 12 > d.size()) return 1;
    const uint32_t len = u32(d.data() + o), isize = u32(d.data() + o + 4), want = u32(d.data() + o + 8);
    o += 12;
    if (o + len + (want ? isize : 0) > d.size()) return 1;
    std::unique_ptr<uint8_t[]> in(new uint8_t[len]), out(new uint8_t[isize]), zout(new uint8_t[isize]);
    if (len) memcpy(in.get(), d.data() + o, len);
    o += len;
    const uint8_t* expect = d.data() + o;
    if (want) o += isize;
    const int32_t st = uc::inflate_block(in.get(), len, out.get(), isize);
    const bool z = zlib_accepts(in.get(), len, zout.get(), isize);
    if (st < 0 || st >= uc::inf::kNumStatus) {
      printf("bad %u status %d\n", i, st);
      bad++;
      continue;
    }
    cls[st]++;
    accepted += st == 0;
    if ((st == 0) != (want != 0) || z != (want != 0)) {
      printf("bad %u status %d (%s), zlib %d, the case file %u\n", i, st, uc::inf::status_name(st), (int)z, want);
      bad++;
    } else if (want && isize && (memcmp(out.get(), expect, isize) || memcmp(zout.get(), expect, isize))) {
      printf("bad %u bytes differ\n", i);
      bad++;
    }
  }
  printf("blocks=%u accepted=%ld rejected=%ld bad=%ld\n", n, accepted, (long)n - accepted, bad);
  for (int k = 0; k < uc::inf::kNumStatus; k++) printf("class %d %ld\n", k, cls[k]);
  return bad ? 3 : 0;
}
