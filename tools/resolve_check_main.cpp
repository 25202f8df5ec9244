// resolve_check_main.cpp -- host-only driver of resolve.cpp's resolve_block for tests/test_resolve_cpu.py (test
// infrastructure, no GPU, no HIP).
//
// The test writes what a pass hands the host -- HostQs and records built by tests/pass_ref.py -- and a table of
// round-B answers; this calls resolve_block once per configuration and prints everything it decided, for the test to
// compare with tests/resolve_ref.py's greedy_block.  Unlike the ThreadSanitizer replay (resolve_tsan_main.cpp)
// nothing here was ever produced by resolve_block itself.
//
// Input: whitespace-separated integers.
//   acc[kTabL * kTabM] rank[kTabL * kTabM] ncases, then per case
//   q0 nq w0 s0 both o4_T maxaccepts maxrejects nbins [bin_s[nbins] hqbin[q0 + nq]]
//   hlen[q0 + nq]  state[q0 - w0]
//   per query-strand: best_t cells rec best_rank w flags nrel e npeer rel[kInlineRel]
//   nrecs recs[nrecs]  nans (pq pt res)[nans]
//   nconf (pre_resolve pre_spec par_inorder par_min threads)[nconf]
// Output: "case", then per configuration
//   R rc | states | targets | strands | new centroids | n_alignments cells
//   S n_deferred pairs_round_b n_merged_walks round-B trips, largest trip | kind histogram 0..5 | pq:pt of every round-B pair asked for
//   K the kind of every query-strand, one digit each
//   E pq pt            a round-B pair missing from the table
// States, targets and strands are the block's; a query that is no member prints target -1 and strand 0 (they are
// initialised so and must stay so).
//
// Usage: resolve_check <input.txt>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../ont-tcrconsensus_amd/csrc/resolve.h"

using namespace uc;

namespace {

struct In {
  FILE* f;
  bool ok = true;
  int64_t get() {
    long long v = 0;
    if (fscanf(f, "%lld", &v) != 1) ok = false;
    return v;
  }
  template <typename T>
  std::vector<T> vec(int64_t n) {
    std::vector<T> v((size_t)(n > 0 ? n : 0));
    for (auto& x : v) x = (T)get();
    return v;
  }
};

template <typename T>
void print_vec(const std::vector<T>& v) {
  for (const auto& x : v) printf(" %lld", (long long)x);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: resolve_check <input.txt>\n");
    return 2;
  }
  In in{fopen(argv[1], "r")};
  if (!in.f) {
    fprintf(stderr, "%s: cannot open\n", argv[1]);
    return 2;
  }
  const std::vector<uint8_t> acc = in.vec<uint8_t>((int64_t)kTabL * kTabM);
  const std::vector<uint16_t> rank = in.vec<uint16_t>((int64_t)kTabL * kTabM);
  const int64_t ncases = in.get();
  std::map<int, std::unique_ptr<WorkPool>> pools;  // one pool per thread count, kept over the cases
  for (int64_t cs = 0; cs < ncases && in.ok; cs++) {
    const int32_t q0 = (int32_t)in.get(), nq = (int32_t)in.get(), w0 = (int32_t)in.get(), s0 = (int32_t)in.get();
    const int both = (int)in.get();
    const int32_t o4_T = (int32_t)in.get();
    const int maxaccepts = (int)in.get(), maxrejects = (int)in.get();
    const int64_t nbins = in.get();
    if (!in.ok || q0 < 0 || nq < 0 || w0 < s0 || w0 > q0 || s0 < 0 || both < 1 || both > 2 || nbins < 0) break;
    std::vector<int32_t> bin_s, hqbin;
    if (nbins) {
      bin_s = in.vec<int32_t>(nbins);
      hqbin = in.vec<int32_t>((int64_t)q0 + nq);
    }
    const std::vector<uint8_t> hlen = in.vec<uint8_t>((int64_t)q0 + nq);
    const std::vector<uint8_t> state_in = in.vec<uint8_t>((int64_t)q0 - w0);
    std::vector<HostQs> hq((size_t)nq * both);
    for (HostQs& h : hq) {
      h.best_t = (uint32_t)in.get();
      h.cells = (uint32_t)in.get();
      h.rec = (uint32_t)in.get();
      h.best_rank = (uint16_t)in.get();
      h.w = (uint8_t)in.get();
      h.flags = (uint8_t)in.get();
      h.nrel = (uint16_t)in.get();
      h.e = (uint8_t)in.get();
      h.npeer = (uint8_t)in.get();
      for (int i = 0; i < kInlineRel; i++) h.rel[i] = (uint16_t)in.get();
    }
    std::vector<uint32_t> recs = in.vec<uint32_t>(in.get());
    recs.resize(recs.size() + kRecWords, 0);  // a corrupt record's counts may point past its end
    std::unordered_map<uint64_t, uint32_t> answers;
    for (int64_t n = in.get(), i = 0; i < n && in.ok; i++) {
      const uint64_t pq = (uint64_t)in.get(), pt = (uint64_t)in.get();
      answers[pq << 32 | pt] = (uint32_t)in.get();
    }
    const int64_t nconf = in.get();
    printf("case\n");
    for (int64_t cf = 0; cf < nconf && in.ok; cf++) {
      ResolveEnv env;
      env.pre_resolve = in.get() != 0;
      env.pre_spec = in.get() != 0;
      env.par_inorder = in.get() != 0;
      env.par_min = (int)in.get();
      const int threads = (int)in.get();
      if (!in.ok || threads < 1 || threads > 64) break;
      // the bin's states: [s0, w0) final before the window (never read), the window as given, the block undetermined
      std::vector<uint8_t> st_buf((size_t)(q0 + nq - s0), ST_MEMBER);
      for (int32_t x = w0; x < q0; x++) st_buf[(size_t)(x - s0)] = state_in[(size_t)(x - w0)];
      for (int32_t x = q0; x < q0 + nq; x++) st_buf[(size_t)(x - s0)] = ST_UNDET;
      StateView state{st_buf.data(), s0};
      std::vector<int32_t> target((size_t)(q0 + nq), -1);
      std::vector<uint8_t> strand((size_t)(q0 + nq), 0);
      env.hlen = hlen.data();
      env.acc = acc.data();
      env.rank = rank.data();
      env.both = both;
      env.o4_T = o4_T;
      env.maxaccepts = maxaccepts;
      env.maxrejects = maxrejects;
      env.hqbin = nbins ? hqbin.data() : nullptr;
      env.bin_s = nbins ? bin_s.data() : nullptr;
      env.target = target.data();
      env.strand = strand.data();
      std::vector<uint32_t> asked_q, asked_t;
      std::vector<std::pair<uint32_t, uint32_t>> missing;
      int trips = 0;
      size_t largest = 0;
      RoundB rb = [&](const std::vector<uint32_t>& pq, const std::vector<uint32_t>& pt, std::vector<uint32_t>& res) {
        trips++;
        largest = std::max(largest, pq.size());
        for (size_t x = 0; x < pq.size(); x++) {
          asked_q.push_back(pq[x]);
          asked_t.push_back(pt[x]);
          const auto it = answers.find((uint64_t)pq[x] << 32 | pt[x]);
          if (it == answers.end()) missing.push_back({pq[x], pt[x]});
          res[x] = it == answers.end() ? 0 : it->second;
        }
      };
      auto& pool = pools[threads];
      if (!pool) pool.reset(new WorkPool(threads));
      ResolveScratch scr;
      ResolveStats rs;
      std::vector<int32_t> cents;
      const int rc = resolve_block(env, q0, nq, w0, hq.data(), recs.data(), state, scr, *pool, cents, rs, rb);
      printf("R %d |", rc);
      for (int32_t x = q0; x < q0 + nq; x++) printf(" %d", (int)st_buf[(size_t)(x - s0)]);
      printf(" |");
      for (int32_t x = q0; x < q0 + nq; x++) printf(" %d", (int)target[(size_t)x]);
      printf(" |");
      for (int32_t x = q0; x < q0 + nq; x++) printf(" %d", (int)strand[(size_t)x]);
      printf(" |");
      print_vec(cents);
      printf(" | %lld %lld\n", (long long)rs.n_alignments, (long long)rs.cells);
      int64_t hist[6] = {0, 0, 0, 0, 0, 0};
      if (rc != kResolveOverflow)
        for (size_t qs = 0; qs < (size_t)nq * both && qs < scr.kind.size(); qs++)
          if (scr.kind[qs] < 6) hist[scr.kind[qs]]++;
      printf("S %lld %lld %lld %d %zu |", (long long)rs.n_deferred, (long long)rs.pairs_round_b,
             (long long)rs.n_merged_walks, trips, largest);
      for (int k = 0; k < 6; k++) printf(" %lld", (long long)hist[k]);
      printf(" |");
      for (size_t x = 0; x < asked_q.size(); x++) printf(" %u:%u", asked_q[x], asked_t[x]);
      printf("\n");
      printf("K ");
      if (rc != kResolveOverflow)
        for (size_t qs = 0; qs < (size_t)nq * both && qs < scr.kind.size(); qs++) printf("%d", (int)scr.kind[qs]);
      printf("\n");
      for (const auto& m : missing) printf("E %u %u\n", m.first, m.second);
    }
  }
  fclose(in.f);
  if (!in.ok) {
    fprintf(stderr, "%s: truncated or malformed input\n", argv[1]);
    return 2;
  }
  return 0;
}
