// deflate_check_main.cpp -- drives the HIP-free DEFLATE encoder (ont-tcrconsensus_amd/csrc/deflate.h) under ASan +
// UBSan, without a GPU (make deflate_check; tests/test_bgzf_deflate_cpu.py; tests/test_gpu_bgzf_deflate.py builds it
// without the sanitizers, DEFLATE_SAN=, and compares the kernel's bytes with the file it writes).  uc::deflate_block
// is the host restatement of k_bgzf_deflate.
//
//   deflate_check cases <file> [<out.bgzf>]
//       <file> = u32 count, then per case `u32 bytes` and the bytes (tests/deflate_cases.py write_case_file).  Each
//       case is cut into 0xff00-byte blocks; every block's input, output (n + 5 bytes) and token store (n words) is a
//       heap block of exactly its size, so a byte read or written past either is a sanitizer report.  Every block's
//       payload must be at most n + 5 bytes and inflate to the input with C zlib and with uc::inflate_block, and each
//       code set it built must be complete or the single code of one bit (the distance set may have none).  Prints
//       `bad ...` per difference, `block <case> <k> kind=<0|1|2> bytes=<payload> tokens=<t> flags=<f>` per block,
//       `case <i> off=<o> size=<s>` per case (its BGZF, EOF block included, in <out.bgzf>), then
//       `cases=<n> blocks=<b> bad=<x>`; exit 0 iff bad=0.
//   deflate_check builder
//       the code builder on hand-made histograms: `builder <name> used=<m> max=<longest> limited=<0|1> kraft=<sum of
//       2^(limit - len)>/<2^limit>` per histogram, and `bad ...` for a set that is neither complete nor the single code
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../ont-tcrconsensus_amd/csrc/deflate.h"

namespace {
using namespace uc;
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
bool zlib_inflates(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t isize) {
  z_stream zs{};
  if (inflateInit2(&zs, -15) != Z_OK) return false;
  zs.next_in = const_cast<Bytef*>(in);
  zs.avail_in = n;
  zs.next_out = out;
  zs.avail_out = isize;
  const int rc = inflate(&zs, Z_FINISH);
  const bool ok = rc == Z_STREAM_END && zs.avail_out == 0 && zs.avail_in == 0;
  inflateEnd(&zs);
  return ok;
}
// the Kraft sum of lens[0 .. n) in units of 2^-15, the number of codes and the longest
struct Kraft {
  uint32_t sum = 0, used = 0, longest = 0;
};
Kraft kraft(const uint8_t* lens, int n) {
  Kraft k;
  for (int s = 0; s < n; s++)
    if (lens[s]) {
      k.sum += 1u << (15 - lens[s]);
      k.used++;
      if (lens[s] > k.longest) k.longest = lens[s];
    }
  return k;
}
// complete, or the single code of one bit, or (none_ok) no code at all
bool set_ok(const Kraft& k, uint32_t limit, bool single_ok, bool none_ok) {
  if (k.longest > limit) return false;
  if (k.used == 0) return none_ok;
  if (k.sum == 1u << 15) return true;
  return single_ok && k.used == 1 && k.longest == 1;
}
const uint8_t kEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                          0x02, 0,    0x1b, 0,    0x03, 0, 0, 0, 0, 0, 0, 0,    0,    0};

int run_builder() {
  struct Case {
    const char* name;
    int nsym, limit, min_codes;
    std::vector<uint32_t> hist;
  };
  std::vector<Case> cases;
  std::vector<uint32_t> fib(286), eq(286, 7), one(286, 0), two(286, 0), eob(286, 0);
  uint32_t a = 1, b = 1;
  for (int s = 0; s < 286; s++) {  // Fibonacci, saturating: the unlimited depth is far past 15
    fib[s] = a;
    const uint64_t c = (uint64_t)a + b;
    a = b, b = c > 0x3fffffu ? 0x3fffffu : (uint32_t)c;
  }
  one[65] = 9, one[256] = 0;
  two[65] = 3, two[256] = 1;
  eob[256] = 1;
  cases.push_back({"fibonacci", 286, 15, 1, fib});
  cases.push_back({"equal", 286, 15, 1, eq});
  cases.push_back({"one", 286, 15, 1, one});
  cases.push_back({"two", 286, 15, 1, two});
  cases.push_back({"only256", 286, 15, 1, eob});
  cases.push_back({"clen_fibonacci", 19, 7, 2, {1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181}});
  cases.push_back({"clen_one", 19, 7, 2, {0, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}});
  cases.push_back({"dist_none", 30, 15, 1, std::vector<uint32_t>(30, 0)});
  int bad = 0;
  for (const Case& c : cases) {
    std::unique_ptr<dfl::Work> W(new dfl::Work);
    std::unique_ptr<uint32_t[]> hist(new uint32_t[c.nsym]);
    std::unique_ptr<uint8_t[]> lens(new uint8_t[c.nsym]);
    memcpy(hist.get(), c.hist.data(), (size_t)c.nsym * 4);
    dfl::HostIo io{nullptr, nullptr, 0, nullptr, 0, 0};
    const uint32_t limited = dfl::build_lengths(io, W->c.b, hist.get(), c.nsym, c.limit, c.min_codes, lens.get());
    const Kraft k = kraft(lens.get(), c.nsym);
    uint32_t used = 0;
    for (int s = 0; s < c.nsym; s++) {
      used += c.hist[s] != 0;
      if (c.hist[s] && !lens[s]) printf("bad builder %s: symbol %d has no code\n", c.name, s), bad++;
    }
    // a rarer symbol never has a shorter code
    for (int s = 0; s < c.nsym; s++)
      for (int t = 0; t < c.nsym; t++)
        if (c.hist[s] && c.hist[t] && c.hist[s] < c.hist[t] && lens[s] < lens[t])
          printf("bad builder %s: %d (x%u) shorter than %d (x%u)\n", c.name, s, c.hist[s], t, c.hist[t]), bad++;
    if (!set_ok(k, (uint32_t)c.limit, c.min_codes == 1, used == 0)) printf("bad builder %s: code set\n", c.name), bad++;
    printf("builder %s used=%u max=%u limited=%u kraft=%u/%u\n", c.name, used, k.longest, limited, k.sum >> (15 - c.limit),
           1u << c.limit);
  }
  printf("builder bad=%d\n", bad);
  return bad ? 3 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "builder")) return run_builder();
  if (argc < 3 || argc > 4 || strcmp(argv[1], "cases")) {
    fprintf(stderr, "usage: deflate_check cases <file> [<out.bgzf>] | deflate_check builder\n");
    return 1;
  }
  std::vector<uint8_t> d, file;
  if (!read_file(argv[2], d) || d.size() < 4) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 1;
  }
  const uint32_t ncase = u32(d.data());
  size_t o = 4;
  long bad = 0, blocks = 0;
  std::unique_ptr<dfl::Work> W(new dfl::Work);
  for (uint32_t i = 0; i < ncase; i++) {
    if (o + 4 > d.size()) return 1;
    const uint32_t len = u32(d.data() + o);
    o += 4;
    if (o + len > d.size()) return 1;
    const size_t case_off = file.size();
    for (uint32_t a = 0, k = 0; a < len; a += dfl::kMaxBlock, k++, blocks++) {
      const uint32_t n = len - a < dfl::kMaxBlock ? len - a : dfl::kMaxBlock;
      std::unique_ptr<uint8_t[]> in(new uint8_t[n]), out(new uint8_t[n + 5]), z(new uint8_t[n]), h(new uint8_t[n]);
      std::unique_ptr<uint32_t[]> tok(new uint32_t[n]);
      memcpy(in.get(), d.data() + o + a, n);
      dfl::Result R;
      if (!deflate_block(in.get(), n, out.get(), tok.get(), *W, R) || R.kind > 2) {
        printf("bad %u %u the encoder failed (bytes %u of %u)\n", i, k, R.bytes, n + 5);
        bad++;
        continue;
      }
      printf("block %u %u kind=%u bytes=%u tokens=%u flags=%u\n", i, k, R.kind, R.bytes, R.ntok, R.flags);
      if (!zlib_inflates(out.get(), R.bytes, z.get(), n) || memcmp(z.get(), in.get(), n))
        printf("bad %u %u zlib does not give the input back\n", i, k), bad++;
      const int32_t st = inflate_block(out.get(), R.bytes, h.get(), n);
      if (st || memcmp(h.get(), in.get(), n)) printf("bad %u %u inflate_block: status %d\n", i, k, st), bad++;
      const dfl::Codes& C = W->c;
      if (!set_ok(kraft(C.lens, (int)C.hlit), 15, true, false) || !C.lens[256])
        printf("bad %u %u literal/length code set\n", i, k), bad++;
      if (!set_ok(kraft(C.lens + C.hlit, (int)C.hdist), 15, true, true)) printf("bad %u %u distance code set\n", i, k), bad++;
      if (!set_ok(kraft(C.clen, 19), 7, false, false)) printf("bad %u %u code-length code set\n", i, k), bad++;
      const uint8_t hdr[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};
      const uint32_t total = R.bytes + 26, crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), in.get(), n);
      file.insert(file.end(), hdr, hdr + 16);
      file.push_back((uint8_t)((total - 1) & 0xff)), file.push_back((uint8_t)((total - 1) >> 8));
      file.insert(file.end(), out.get(), out.get() + R.bytes);
      for (int x = 0; x < 4; x++) file.push_back((uint8_t)(crc >> (8 * x)));
      for (int x = 0; x < 4; x++) file.push_back((uint8_t)(n >> (8 * x)));
    }
    file.insert(file.end(), kEof, kEof + 28);
    printf("case %u off=%zu size=%zu\n", i, case_off, file.size() - case_off);
    o += len;
  }
  printf("cases=%u blocks=%ld bad=%ld\n", ncase, blocks, bad);
  if (argc == 4) {
    FILE* f = fopen(argv[3], "wb");
    if (!f || (file.size() && fwrite(file.data(), 1, file.size(), f) != file.size()) || fclose(f) != 0) {
      fprintf(stderr, "cannot write %s\n", argv[3]);
      return 1;
    }
  }
  return bad ? 3 : 0;
}
