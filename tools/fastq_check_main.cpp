// fastq_check_main.cpp -- drives the HIP-free side of the fastq_filter drop-in (ont-tcrconsensus_amd/csrc/
// fastq_filter.cpp) under ASan + UBSan, without a GPU (make fastq_check; tests/test_fastq_filter_cpu.py).  The device
// is replaced by fq::HostBackend, the host restatement of the kernels: per record the sum of the fixed-point table and
// the smallest / largest byte, and in stats mode the five counts of the statistics tables.
//
//   fastq_check filter <in> <out|-> <discarded|-> <log|-> <threads> <chunk> <ascii> <qmin> <qmax> <minlen> <maxlen>
//                      <maxee> <maxee_rate>
//       runs the whole step; prints `rc=<n_kept or error code>`, one `name=value` line per result counter and `err=<message>`
//   fastq_check stats <in> <out|-> <discarded|-> <log|-> <before_txt|-> <after_txt|-> <threads> <chunk> <ascii> <qmin>
//                     <qmax> <minlen> <maxlen> <maxee> <maxee_rate>
//       the same step in stats mode (row f5b): the gathered sequence bytes, the host restatement of k_fastq_stats,
//       the two accumulators, the histogram walk and the formatter; writes the two `seqkit stat -a` tables and prints,
//       after the lines above, `before.<name>=<value>` and `after.<name>=<value>` for every integer of the two
//       umiclust_fastq_stats and the doubles in hexadecimal
//   fastq_check seams <in>
//       indexes the file in windows of every length from 1 byte to the whole file, on 1, 2, 3 and 7 threads (so a
//       slice boundary falls on every byte), and compares each pass with the one-window, one-thread index; prints
//       `seams ok <passes> records=<n> fallback=<passes that left the 4-line path>`
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../ont-tcrconsensus_amd/csrc/fastq_filter.h"

using namespace uc;

namespace {

const char* opt_path(const char* s) { return strcmp(s, "-") == 0 ? nullptr : s; }

struct Flat {  // a record by value, whatever chunk and arena it came from
  int64_t begin, end, len;
  std::string label, seq, qual;
  bool operator==(const Flat& o) const {
    return begin == o.begin && end == o.end && len == o.len && label == o.label && seq == o.seq && qual == o.qual;
  }
};

void flatten(const std::string& data, const std::vector<fq::Rec>& recs, const std::vector<char>& arena,
             std::vector<Flat>& out) {
  for (const fq::Rec& r : recs) {
    const char* base = r.arena ? arena.data() : data.data();
    Flat f{r.begin, r.end, r.len, data.substr((size_t)r.label, (size_t)r.label_len),
           std::string(base + r.seq, (size_t)r.len), std::string(base + r.qual, (size_t)r.len)};
    if (r.verbatim && data.substr((size_t)r.begin, (size_t)(r.end - r.begin)) != "@" + f.label + "\n" + f.seq + "\n+\n" + f.qual + "\n") {
      fprintf(stderr, "record at %lld is marked verbatim but is not in output form\n", (long long)r.begin);
      exit(3);
    }
    out.push_back(f);
  }
}

int seams(const char* path) {
  std::ifstream in(path, std::ios::binary);
  std::stringstream ss;
  ss << in.rdbuf();
  const std::string data = ss.str();
  const int64_t size = (int64_t)data.size();
  std::vector<fq::Rec> recs;
  std::vector<char> arena;
  std::vector<Flat> want;
  std::string err;
  int64_t next = 0;
  bool ml = false;
  const int rc0 = fq::index_window(data.data(), size, 0, size, 1, recs, arena, &next, &ml, err);
  flatten(data, recs, arena, want);
  long passes = 0, fallback = 0;
  const int Ts[4] = {1, 2, 3, 7};
  for (int T : Ts)
    for (int64_t W = 1; W <= size + 1; W++) {
      std::vector<Flat> got;
      bool multi = false;
      int rc = UMICLUST_OK;
      for (int64_t pos = 0; pos < size && rc == UMICLUST_OK;) {
        rc = fq::index_window(data.data(), size, pos, pos + W, T, recs, arena, &next, &multi, err);
        flatten(data, recs, arena, got);
        if (rc == UMICLUST_OK && next <= pos) {
          fprintf(stderr, "no progress at %lld (W %lld, T %d)\n", (long long)pos, (long long)W, T);
          return 2;
        }
        pos = next;
      }
      if (rc != rc0 || !(got == want)) {
        fprintf(stderr, "index differs: W %lld, T %d: rc %d vs %d, %zu vs %zu records\n", (long long)W, T, rc, rc0,
                got.size(), want.size());
        return 2;
      }
      passes++;
      fallback += multi;
    }
  printf("seams ok %ld records=%zu fallback=%ld rc=%d\n", passes, want.size(), fallback, rc0);
  return 0;
}

void print_stats(const char* which, const umiclust_fastq_stats& t) {
  const long long v[11] = {t.num_seqs, t.sum_len, t.min_len, t.max_len, t.n50,    t.n50_num,
                           t.n_q20,    t.n_q30,   t.n_gc,    t.sum_n,   t.sum_gap};
  static const char* names[11] = {"num_seqs", "sum_len", "min_len", "max_len", "n50",    "n50_num",
                                  "n_q20",    "n_q30",   "n_gc",    "sum_n",   "sum_gap"};
  for (int k = 0; k < 11; k++) printf("%s.%s=%lld\n", which, names[k], v[k]);
  printf("%s.ee_fx_lo=%llu\n%s.ee_fx_hi=%llu\n%s.type=%d\n", which, (unsigned long long)t.ee_fx_lo, which,
         (unsigned long long)t.ee_fx_hi, which, t.type);
  printf("%s.avg_len=%a\n%s.q1=%a\n%s.q2=%a\n%s.q3=%a\n", which, t.avg_len, which, t.q1, which, t.q2, which, t.q3);
  printf("%s.q20_pct=%a\n%s.q30_pct=%a\n%s.avg_qual=%a\n%s.gc_pct=%a\n", which, t.q20_pct, which, t.q30_pct, which,
         t.avg_qual, which, t.gc_pct);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "seams") == 0) return seams(argv[2]);
  const bool stats = argc == 17 && strcmp(argv[1], "stats") == 0;
  if (!stats && (argc != 15 || strcmp(argv[1], "filter") != 0)) {
    fprintf(stderr, "usage: fastq_check filter <in> <out|-> <discarded|-> <log|-> <threads> <chunk> <ascii> <qmin> "
                    "<qmax> <minlen> <maxlen> <maxee> <maxee_rate> | fastq_check stats <in> <out|-> <discarded|-> "
                    "<log|-> <before_txt|-> <after_txt|-> <threads> ... <maxee_rate> | fastq_check seams <in>\n");
    return 1;
  }
  fq::Paths paths;
  paths.in = argv[2];
  paths.out = opt_path(argv[3]);
  paths.discarded = opt_path(argv[4]);
  paths.log = opt_path(argv[5]);
  umiclust_fastq_stats before, after;
  fq::StatsReq req;
  if (stats) {
    req.before_txt = opt_path(argv[6]);
    req.after_txt = opt_path(argv[7]);
    req.before = &before;
    req.after = &after;
    argv += 2;  // the filter's own arguments follow
  }
  const int threads = atoi(argv[6]);
  const int64_t chunk = atoll(argv[7]);
  umiclust_fastq_filter_params p;
  memset(&p, 0, sizeof(p));
  p.fastq_ascii = atoi(argv[8]);
  p.fastq_qmin = atoi(argv[9]);
  p.fastq_qmax = atoi(argv[10]);
  p.fastq_minlen = atoi(argv[11]);
  p.fastq_maxlen = atoi(argv[12]);
  p.fastq_maxee = atof(argv[13]);
  p.fastq_maxee_rate = atof(argv[14]);
  fq::HostBackend be;
  umiclust_fastq_filter_result r;
  std::string err;
  const int64_t rc = fq::run_filter(p, paths, threads, chunk, be, &r, err, stats ? &req : nullptr);
  printf("rc=%lld\n", (long long)rc);
  printf("n_input=%lld\nn_kept=%lld\nn_discarded=%lld\nbases_in=%lld\nbases_kept=%lld\n", (long long)r.n_input,
         (long long)r.n_kept, (long long)r.n_discarded, (long long)r.bases_in, (long long)r.bases_kept);
  printf("n_short=%lld\nn_long=%lld\nn_maxee=%lld\nn_maxee_rate=%lld\nn_host_rechecked=%lld\nn_chunks=%lld\n",
         (long long)r.n_short, (long long)r.n_long, (long long)r.n_maxee, (long long)r.n_maxee_rate,
         (long long)r.n_host_rechecked, (long long)r.n_chunks);
  printf("ee_in=%a\nee_kept=%a\n", r.ee_in, r.ee_kept);
  printf("err=%s\n", err.c_str());
  if (stats) {
    print_stats("before", before);
    print_stats("after", after);
  }
  return 0;
}
