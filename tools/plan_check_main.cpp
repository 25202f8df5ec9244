// plan_check_main.cpp -- stand-alone driver of csrc/plan.cpp for the CPU suite (tests/test_plan_cpu.py), built with
// ASan + UBSan.  Reads whitespace-separated integers from a file, any number of cases one after another, and prints
// what the planner / the numbering / the traceback plan makes of each.
//
//   plan_check blocks FILE    case: B mix o4_T regrow b_hint pack bin0 nbins  bin_s[nbins + 1]  hlen[bin_s[nbins]]
//                                   nops  then per op:  0 k (overflowed)  |  1 k D max_npeer (resolved)  |  2 q (halve)
//     prints "case", then after the start and after every op one line:  ret b_eff clean : first,n first,n ...
//   plan_check number FILE    case: sort pack bin0 nbins  bin_s[nbins + 1]  K cent[K]  target[bin_s[0] .. bin_s[nbins])
//     prints "case", then the lines cno, rank_of, ocl, ostart, omemb, bin_k
//   plan_check trace FILE     case: lo hi x0 n  hlen[n]  target[n]  strand[n]   (seqnos 0 .. n - 1, lo <= hi <= n)
//     prints "case", then the lines tp (x0 n1 n2 maxq1 maxq2), slot (of the seqnos [lo, hi); -1: left alone), pq and
//     pt (of the slots given out), maxl (traceback_maxl of [lo, hi))
// Seqnos are absolute: the bins cover [bin_s[0], bin_s[nbins]) and hlen starts at seqno 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ont-tcrconsensus_amd/csrc/plan.h"

using namespace uc;

namespace {

struct Reader {
  FILE* f;
  bool next(long& v) { return fscanf(f, "%ld", &v) == 1; }
  long get() {
    long v;
    if (!next(v)) {
      fprintf(stderr, "plan_check: truncated input\n");
      exit(2);
    }
    return v;
  }
};

// the bins of a case: bin_s indexed by absolute bin number, hqbin by absolute seqno
struct Bins {
  int32_t bin0 = 0, nbins = 1, s0 = 0, s1 = 0;
  std::vector<int32_t> bin_s, hqbin;
  void read(Reader& in) {
    bin0 = (int32_t)in.get();
    nbins = (int32_t)in.get();
    bin_s.assign((size_t)bin0 + nbins + 1, 0);
    for (int32_t b = 0; b <= nbins; b++) bin_s[bin0 + b] = (int32_t)in.get();
    s0 = bin_s[bin0];
    s1 = bin_s[bin0 + nbins];
    hqbin.assign((size_t)s1, -1);
    for (int32_t b = bin0; b < bin0 + nbins; b++)
      for (int32_t s = bin_s[b]; s < bin_s[b + 1]; s++) hqbin[s] = b;
  }
};

void print_vec(const char* name, const int32_t* p, size_t n) {
  printf("%s", name);
  for (size_t i = 0; i < n; i++) printf(" %d", p[i]);
  printf("\n");
}

void print_plan(int ret, const BlockPlan& p) {
  printf("%d %d %d :", ret, p.b_eff, p.clean);
  for (const auto& b : p.blocks) printf(" %d,%d", b.first, b.second);
  printf("\n");
}

void blocks_case(Reader& in, long B) {
  BlockPlan p;
  p.B = (int32_t)B;
  p.mix = in.get() != 0;
  p.o4_T = (int32_t)in.get();
  p.regrow = (int32_t)in.get();
  const int32_t b_hint = (int32_t)in.get();
  const bool pack = in.get() != 0;
  Bins bins;
  bins.read(in);
  std::vector<uint8_t> hlen((size_t)bins.s1);
  for (auto& x : hlen) x = (uint8_t)in.get();
  p.hlen = hlen.data();
  p.s0 = bins.s0;
  p.s1 = bins.s1;
  if (pack) {
    p.hqbin = bins.hqbin.data();
    p.bin_s = bins.bin_s.data();
  }
  printf("case\n");
  p.start(b_hint);
  print_plan(0, p);
  for (long nops = in.get(); nops > 0; nops--) {
    const long op = in.get();
    int ret = 0;
    if (op == 0) {
      p.overflowed((int32_t)in.get());
    } else if (op == 1) {
      const int32_t k = (int32_t)in.get();
      const int D = (int)in.get();
      ret = p.resolved(k, D, (int32_t)in.get());
    } else {
      ret = p.halve((int32_t)in.get());
    }
    print_plan(ret, p);
  }
}

void number_case(Reader& in, long sort) {
  const bool pack = in.get() != 0;
  Bins bins;
  bins.read(in);
  std::vector<int32_t> cent((size_t)in.get());
  for (auto& x : cent) x = (int32_t)in.get();
  std::vector<int32_t> target((size_t)bins.s1, -7), cno((size_t)bins.s1, -7), ocl((size_t)bins.s1, -7);
  for (int32_t s = bins.s0; s < bins.s1; s++) target[s] = (int32_t)in.get();
  ClusterNumbers out;
  number_clusters(bins.s0, bins.s1, cent, target.data(), sort != 0, pack ? bins.hqbin.data() : nullptr, bins.bin0,
                  bins.nbins, cno.data(), ocl.data(), out);
  const size_t n = (size_t)(bins.s1 - bins.s0);
  printf("case\n");
  print_vec("cno", cno.data() + bins.s0, n);
  print_vec("rank_of", out.rank_of.data(), out.rank_of.size());
  print_vec("ocl", ocl.data() + bins.s0, n);
  print_vec("ostart", out.ostart.data(), out.ostart.size());
  print_vec("omemb", out.omemb.data(), out.omemb.size());
  print_vec("bin_k", out.bin_k.data(), out.bin_k.size());
}

void trace_case(Reader& in, long lo_) {
  const int32_t lo = (int32_t)lo_, hi = (int32_t)in.get(), x0 = (int32_t)in.get();
  const size_t n = (size_t)in.get();
  std::vector<uint8_t> hlen(n), strand(n);
  std::vector<int32_t> target(n);
  for (auto& x : hlen) x = (uint8_t)in.get();
  for (auto& x : target) x = (int32_t)in.get();
  for (auto& x : strand) x = (uint8_t)in.get();
  size_t members = 0;
  for (int32_t s = lo; s < hi; s++) members += target[s] >= 0;
  // exactly as large as the plan may fill: a slot past the members, or an entry outside [lo, hi), is an ASan report
  std::vector<int32_t> slot((size_t)(hi - lo), -1);
  std::vector<uint32_t> pq((size_t)x0 + members, 0), pt((size_t)x0 + members, 0);
  const TracePlan tp = plan_traceback(hlen.data(), target.data(), strand.data(), lo, hi, x0, slot.data(), pq.data(),
                                      pt.data());
  printf("case\n");
  printf("tp %d %d %d %d %d\n", tp.x0, tp.n1, tp.n2, tp.maxq1, tp.maxq2);
  print_vec("slot", slot.data(), slot.size());
  printf("pq");
  for (size_t x = (size_t)x0; x < pq.size(); x++) printf(" %u", pq[x]);
  printf("\npt");
  for (size_t x = (size_t)x0; x < pt.size(); x++) printf(" %u", pt[x]);
  printf("\nmaxl %d\n", traceback_maxl(hlen.data(), lo, hi));
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3 || (strcmp(argv[1], "blocks") && strcmp(argv[1], "number") && strcmp(argv[1], "trace"))) {
    fprintf(stderr, "usage: plan_check blocks|number|trace FILE\n");
    return 2;
  }
  Reader in{fopen(argv[2], "r")};
  if (!in.f) {
    perror(argv[2]);
    return 2;
  }
  const bool blocks = !strcmp(argv[1], "blocks");
  long first;
  while (in.next(first)) {
    if (blocks) blocks_case(in, first);
    else if (!strcmp(argv[1], "number")) number_case(in, first);
    else trace_case(in, first);
  }
  fclose(in.f);
  return 0;
}
