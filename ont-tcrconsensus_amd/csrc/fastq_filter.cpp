// fastq_filter.cpp -- the HIP-free host side of the `vsearch --fastq_filter` drop-in (see fastq_filter.h).
#include "fastq_filter.h"

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <mutex>
#include <new>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/uio.h>
#include <thread>
#include <unistd.h>

#include "host_io.h"  // parallel_for (header only)

namespace uc {
namespace fq {

using io::parallel_for;

namespace {
double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

void build_tables(int ascii, int qmin, int qmax, Tables& t) {
  memset(t.fx, 0, sizeof(t.fx));
  for (double& x : t.p) x = 0.0;
  t.lo = std::max(0, ascii + qmin);
  t.hi = std::min(255, ascii + qmax);
  for (int b = t.lo; b <= t.hi; b++) {
    const int q = b - ascii;
    t.p[b] = pow(10.0, -q / 10.0);  // O7c
    t.fx[b] = (uint64_t)llrint(ldexp(t.p[b], kFxShift));
  }
}

// ------------------------------------------------------------------ the indexer
namespace {

inline const char* find_nl(const char* p, const char* end) {
  return p < end ? (const char*)memchr(p, '\n', (size_t)(end - p)) : nullptr;
}

// One record of the 4-line shape at pos: `@...`, a sequence line, `+...`, a quality line of the sequence's length,
// followed by `@` or the end of the file.  false: not that shape (the general parser decides what it is).
bool parse4(const char* d, int64_t size, int64_t pos, Rec& r, int64_t* next) {
  const char* end = d + size;
  if (pos >= size || d[pos] != '@') return false;
  const char* e0 = find_nl(d + pos, end);
  if (!e0) return false;
  const char* s1 = e0 + 1;
  const char* e1 = find_nl(s1, end);
  if (!e1) return false;
  const char* s2 = e1 + 1;
  if (s2 >= end || *s2 != '+') return false;
  const char* e2 = find_nl(s2, end);
  if (!e2) return false;
  const char* s3 = e2 + 1;
  const char* e3 = find_nl(s3, end);
  const bool final_nl = e3 != nullptr;
  if (!e3) e3 = end;
  bool cr = false;
  const char* h1 = e0;  // header end without '\r'
  if (h1 > d + pos + 1 && h1[-1] == '\r') h1--, cr = true;
  const char* q1 = e1;
  if (q1 > s1 && q1[-1] == '\r') q1--, cr = true;
  const char* q3 = e3;
  if (q3 > s3 && q3[-1] == '\r') q3--, cr = true;
  if (q1 - s1 != q3 - s3) return false;
  const int64_t nx = final_nl ? (e3 + 1 - d) : size;
  if (nx < size && d[nx] != '@') return false;
  const char* lab = d + pos + 1;
  const char* le = lab;
  while (le < h1 && *le != ' ' && *le != '\t') le++;
  if (le - lab > INT32_MAX) return false;
  r.begin = pos;
  r.end = nx;
  r.label = lab - d;
  r.label_len = (int32_t)(le - lab);
  r.seq = s1 - d;
  r.qual = s3 - d;
  r.len = q1 - s1;
  r.arena = 0;
  r.verbatim = !cr && le == e0 && e2 == s2 + 1 && final_nl;
  *next = nx;
  return true;
}

// The general record (O7a) at pos: blank lines skipped, `@` header, sequence line(s) up to the `+` line, quality
// line(s) up to the sequence length.  1 a record, 0 the end of the file, -1 malformed (err set).
int parse_general(const char* d, int64_t size, int64_t pos, Rec& r, std::vector<char>& arena, int64_t* next,
                  std::string& err) {
  const char* end = d + size;
  const char* p = d + pos;
  while (p < end && (*p == '\n' || *p == '\r')) p++;
  if (p >= end) {
    *next = size;
    return 0;
  }
  auto fail = [&](const char* what) {
    err = std::string("malformed FASTQ: ") + what + " in the record at byte " + std::to_string(p - d);
    return -1;
  };
  if (*p != '@') return fail("a record does not start with '@'");
  r.begin = p - d;
  auto line = [&](const char* s, const char** b, const char** e) {  // [*b, *e) without the line end; returns the next line
    const char* nl = find_nl(s, end);
    const char* le = nl ? nl : end;
    *b = s;
    *e = (le > s && le[-1] == '\r') ? le - 1 : le;
    return nl ? nl + 1 : end;
  };
  const char *b, *e;
  const char* cur = line(p, &b, &e);
  const char* lab = b + 1;
  const char* le = lab;
  while (le < e && *le != ' ' && *le != '\t') le++;
  if (le - lab > INT32_MAX) return fail("a header line is too long");
  r.label = lab - d;
  r.label_len = (int32_t)(le - lab);
  // sequence lines up to the '+' line, then quality lines up to the sequence length
  std::vector<std::pair<const char*, const char*>> sl, ql;
  int64_t slen = 0, qlen = 0;
  bool plus = false;
  while (cur < end) {
    if (*cur == '+') {
      plus = true;
      break;
    }
    cur = line(cur, &b, &e);
    sl.emplace_back(b, e);
    slen += e - b;
  }
  if (!plus) return fail("no '+' line");
  cur = line(cur, &b, &e);
  while (cur < end && qlen < slen) {
    cur = line(cur, &b, &e);
    ql.emplace_back(b, e);
    qlen += e - b;
  }
  if (qlen != slen) return fail("sequence and quality lengths differ");
  r.len = slen;
  r.verbatim = 0;
  r.end = cur - d;
  if (sl.size() <= 1 && ql.size() <= 1) {
    r.arena = 0;
    r.seq = sl.empty() ? r.begin : sl[0].first - d;
    r.qual = ql.empty() ? r.begin : ql[0].first - d;
  } else {  // joined copies: the sequence, then the quality
    r.arena = 1;
    r.seq = (int64_t)arena.size();
    for (auto& x : sl) arena.insert(arena.end(), x.first, x.second);
    r.qual = (int64_t)arena.size();
    for (auto& x : ql) arena.insert(arena.end(), x.first, x.second);
  }
  *next = cur - d;
  return 1;
}

// first verified 4-line record start at or after b (a line start), size at the end of the file, -1: none found
int64_t resync(const char* d, int64_t size, int64_t lo, int64_t b) {
  int64_t c = b;
  if (c > lo && d[c - 1] != '\n') {
    const char* nl = find_nl(d + c, d + size);
    if (!nl) return size;
    c = nl + 1 - d;
  }
  for (int tries = 0; tries < 6; tries++) {
    if (c >= size) return size;
    Rec r;
    int64_t nx;
    if (d[c] == '@' && parse4(d, size, c, r, &nx)) return c;
    const char* nl = find_nl(d + c, d + size);
    if (!nl) return size;
    c = nl + 1 - d;
  }
  return -1;
}

}  // namespace

int index_window(const char* d, int64_t size, int64_t pos, int64_t want_end, int T, std::vector<Rec>& recs,
                 std::vector<char>& arena, int64_t* next, bool* multi_line, std::string& err) {
  recs.clear();
  arena.clear();
  want_end = std::min(want_end, size);
  if (pos >= size) {
    *next = size;
    return UMICLUST_OK;
  }
  if (want_end <= pos) want_end = pos + 1;
  T = (int)std::max<int64_t>(1, std::min<int64_t>(T, (want_end - pos) / 16));
  if (!*multi_line) {
    std::vector<std::vector<Rec>> part((size_t)T);
    std::vector<int64_t> first((size_t)T, -1), last((size_t)T, -1);
    std::vector<uint8_t> bad((size_t)T, 0);
    parallel_for(T, [&](int t) {
      const int64_t lo = pos + (want_end - pos) * t / T, hi = pos + (want_end - pos) * (t + 1) / T;
      int64_t cur = t == 0 ? pos : resync(d, size, pos, lo);
      if (cur < 0) {
        bad[t] = 1;
        return;
      }
      first[t] = cur;
      while (cur < hi && cur < size) {
        Rec r;
        int64_t nx;
        if (!parse4(d, size, cur, r, &nx)) {
          bad[t] = 1;
          return;
        }
        part[t].push_back(r);
        cur = nx;
      }
      last[t] = cur;
    });
    bool ok = true;
    for (int t = 0; t < T && ok; t++) ok = !bad[t] && (t == 0 || first[t] == last[t - 1]);
    if (ok) {
      size_t n = 0;
      for (auto& v : part) n += v.size();
      recs.reserve(n);
      for (auto& v : part) recs.insert(recs.end(), v.begin(), v.end());
      *next = last[T - 1];
      return UMICLUST_OK;
    }
    *multi_line = true;  // not 4-line FASTQ (or malformed): one sequential indexer from here on
  }
  int64_t cur = pos;
  while (cur < want_end) {
    Rec r;
    int64_t nx;
    if (parse4(d, size, cur, r, &nx)) {
      recs.push_back(r);
      cur = nx;
      continue;
    }
    const int rc = parse_general(d, size, cur, r, arena, &nx, err);
    if (rc < 0) {
      *next = cur;
      return UMICLUST_EFORMAT;
    }
    cur = nx;
    if (rc == 0) break;
    recs.push_back(r);
  }
  *next = cur;
  return UMICLUST_OK;
}

// ------------------------------------------------------------------ the host backend
bool HostBackend::reserve(int slot, size_t qual_bytes, size_t nrec, bool stats, Slot& s, std::string&) {
  q[slot].assign(qual_bytes + 2 * kPad, 0);
  offs[slot].assign(nrec + 1, 0);
  ee[slot].assign(nrec + 1, 0);
  lo[slot].assign(nrec + 1, 0);
  hi[slot].assign(nrec + 1, 0);
  slots[slot] = Slot{q[slot].data(), offs[slot].data(), ee[slot].data(), lo[slot].data(), hi[slot].data()};
  if (stats) {
    sq[slot].assign(qual_bytes + 2 * kPad, 0);
    cnt[slot].assign(kCounts * (nrec + 1), 0);
    slots[slot].seq = sq[slot].data();
    slots[slot].cnt = cnt[slot].data();
  }
  s = slots[slot];
  return true;
}

void record_stats(const uint8_t* seq, const uint8_t* qual, int64_t len, const uint64_t* table, int ascii,
                  unsigned __int128* ee, uint8_t* qlo, uint8_t* qhi, uint64_t cnt[kCounts]) {
  unsigned __int128 acc = 0;
  uint8_t mn = 255, mx = 0;
  uint64_t c[kCounts] = {0, 0, 0, 0, 0};
  for (int64_t k = 0; k < len; k++) {
    const uint8_t b = qual[k];
    acc += table[b];
    mn = std::min(mn, b);
    mx = std::max(mx, b);
    c[0] += (int)b - ascii >= 20;
    c[1] += (int)b - ascii >= 30;
    const uint8_t x = seq[k];
    c[2] += x == 'G' || x == 'C' || x == 'g' || x == 'c';
    c[3] += x == 'N' || x == 'n';
    c[4] += x == '-' || x == '.' || x == ' ';
  }
  *ee = acc;
  *qlo = mn;
  *qhi = mx;
  for (int j = 0; j < kCounts; j++) cnt[j] = c[j];
}

bool HostBackend::run_stats(int slot, size_t, int64_t nrec, const uint64_t* table, int ascii, double* t_h2d_s,
                            double* t_kernel_s, std::string&) {
  const Slot& s = slots[slot];
  for (int64_t i = 0; i < nrec; i++) {
    unsigned __int128 acc;
    uint64_t c[kCounts];
    record_stats(s.seq + kPad + s.offs[i], s.qual + kPad + s.offs[i], s.offs[i + 1] - s.offs[i], table, ascii, &acc,
                 &s.qlo[i], &s.qhi[i], c);
    s.ee[i] = (int64_t)acc;
    for (int j = 0; j < kCounts; j++) s.cnt[kCounts * i + j] = (uint32_t)c[j];
  }
  *t_h2d_s = 0.0;
  *t_kernel_s = 0.0;
  return true;
}

bool HostBackend::run(int slot, size_t, int64_t nrec, const uint64_t* table, double* t_h2d_s, double* t_kernel_s,
                      std::string&) {
  const Slot& s = slots[slot];
  for (int64_t i = 0; i < nrec; i++) {
    uint64_t acc = 0;
    uint8_t mn = 255, mx = 0;
    for (int64_t k = s.offs[i]; k < s.offs[i + 1]; k++) {
      const uint8_t b = s.qual[kPad + k];
      acc += table[b];
      mn = std::min(mn, b);
      mx = std::max(mx, b);
    }
    s.ee[i] = (int64_t)acc;
    s.qlo[i] = mn;
    s.qhi[i] = mx;
  }
  *t_h2d_s = 0.0;
  *t_kernel_s = 0.0;
  return true;
}

// ------------------------------------------------------------------ the decision (O7c, O7d)
static int decide_from_ee(const umiclust_fastq_filter_params& p, int64_t len, double ee) {
  if (len < p.fastq_minlen) return 1;
  if (p.fastq_maxlen >= 0 && len > p.fastq_maxlen) return 2;
  if (p.fastq_maxee >= 0.0 && ee > p.fastq_maxee) return 3;
  if (p.fastq_maxee_rate >= 0.0 && len > 0 && ee / (double)len > p.fastq_maxee_rate) return 4;
  return 0;
}

int decide_exact(const umiclust_fastq_filter_params& p, const Tables& t, const uint8_t* qual, int64_t len) {
  double ee = 0.0;
  for (int64_t i = 0; i < len; i++) ee += t.p[qual[i]];  // left to right, in double
  return decide_from_ee(p, len, ee);
}

int decide_fx(const umiclust_fastq_filter_params& p, int64_t len, int64_t ee_fx, int* in_band) {
  *in_band = 0;
  if (len < p.fastq_minlen) return 1;
  if (p.fastq_maxlen >= 0 && len > p.fastq_maxlen) return 2;
  const double ee = ldexp((double)ee_fx, -kFxShift);
  const double n = (double)len;
  // the guard band: the table's rounding, the sequential double sum's, the comparison's
  const double base = n * ldexp(1.0, -41) + 2.0 * n * ldexp(1.0, -53) * ee;
  if (p.fastq_maxee >= 0.0) {
    const double thr = p.fastq_maxee;
    if (fabs(ee - thr) <= base + 4.0 * ldexp(1.0, -52) * thr) {
      *in_band = 1;
      return -1;
    }
    if (ee > thr) return 3;
  }
  if (p.fastq_maxee_rate >= 0.0 && len > 0) {
    const double thr = p.fastq_maxee_rate * n;
    if (fabs(ee - thr) <= base + 4.0 * ldexp(1.0, -52) * thr) {
      *in_band = 1;
      return -1;
    }
    if (ee > thr) return 4;
  }
  return 0;
}

// ------------------------------------------------------------------ the statistics tables (row f5b, policy O8)
int seq_type(const uint8_t* seq, int64_t len) {
  bool dna = true, has_u = false, has_t = false;
  for (int64_t i = 0; i < len; i++) {
    const int c = seq[i] & ~0x20;  // upper case of a letter
    if (c < 'A' || c > 'Z') continue;
    has_u |= c == 'U';
    has_t |= c == 'T';
    dna &= strchr("ACGTRYSWKMBDHVN", c) != nullptr;
  }
  return dna ? 0 : (has_u && !has_t) ? 1 : 2;
}

void StatAcc::add(const uint8_t* seq, int64_t len, unsigned __int128 ee_fx, const uint64_t c[kCounts]) {
  if (num_seqs == 0) type = seq_type(seq, len);
  num_seqs++;
  sum_len += len;
  ee += ee_fx;
  for (int j = 0; j < kCounts; j++) cnt[j] += c[j];
  if (len <= kDevMaxLen) {
    if ((int64_t)hist.size() <= len)
      hist.resize((size_t)std::min<int64_t>(kDevMaxLen + 1, std::max<int64_t>(len + 1, 2 * (int64_t)hist.size())), 0);
    hist[(size_t)len]++;
  } else {
    longer[len]++;
  }
}

namespace {

// the distinct lengths of a histogram in ascending order with their counts
template <typename F>
void walk_up(const StatAcc& a, F f) {
  for (size_t l = 0; l < a.hist.size(); l++)
    if (a.hist[l]) f((int64_t)l, a.hist[l]);
  for (const auto& kv : a.longer) f(kv.first, kv.second);
}

// an integer with thousands commas
std::string commas(uint64_t v) {
  std::string d = std::to_string(v), out;
  for (size_t i = 0; i < d.size(); i++) {
    if (i && (d.size() - i) % 3 == 0) out += ',';
    out += d[i];
  }
  return out;
}

// %.<prec>f of a non-negative number, the integer part with thousands commas
std::string fixed(double v, int prec, bool with_commas) {
  char buf[400];
  snprintf(buf, sizeof(buf), "%.*f", prec, v);
  std::string s = buf;
  if (!with_commas) return s;
  const size_t dot = s.find('.');
  const size_t first = s[0] == '-' ? 1 : 0;
  std::string ip = s.substr(first, dot - first), out = s.substr(0, first);
  for (size_t i = 0; i < ip.size(); i++) {
    if (i && (ip.size() - i) % 3 == 0) out += ',';
    out += ip[i];
  }
  return out + s.substr(dot);
}

}  // namespace

void finish_stats(const StatAcc& a, umiclust_fastq_stats* o) {
  memset(o, 0, sizeof(*o));
  o->type = a.type;
  const int64_t n = a.num_seqs;
  if (n == 0) return;  // O8c: every number is 0
  o->num_seqs = n;
  o->sum_len = a.sum_len;
  o->n_q20 = (int64_t)a.cnt[0];
  o->n_q30 = (int64_t)a.cnt[1];
  o->n_gc = (int64_t)a.cnt[2];
  o->sum_n = (int64_t)a.cnt[3];
  o->sum_gap = (int64_t)a.cnt[4];
  o->ee_fx_lo = (uint64_t)a.ee;
  o->ee_fx_hi = (uint64_t)(a.ee >> 64);
  // O8c: the order statistics the three quartiles need (0-based ranks in the ascending lengths), from one walk.
  // The lower half is the first h lengths, the upper half the last h: the middle one of an odd n is in neither.
  const int64_t h = n / 2;
  int64_t want[6] = {(n - 1) / 2, n / 2, 0, 0, 0, 0}, got[6] = {0, 0, 0, 0, 0, 0};
  if (h > 0) {
    want[2] = (h - 1) / 2;
    want[3] = h / 2;
    want[4] = n - h + (h - 1) / 2;
    want[5] = n - h + h / 2;
  }  // n = 1: all three are the one length
  int64_t seen = 0, mn = -1, mx = 0;
  walk_up(a, [&](int64_t len, int64_t count) {
    if (mn < 0) mn = len;
    mx = len;
    for (int k = 0; k < 6; k++)
      if (want[k] >= seen && want[k] < seen + count) got[k] = len;
    seen += count;
  });
  o->min_len = mn;
  o->max_len = mx;
  o->avg_len = (double)a.sum_len / (double)n;
  o->q2 = (double)(got[0] + got[1]) / 2.0;
  o->q1 = (double)(got[2] + got[3]) / 2.0;
  o->q3 = (double)(got[4] + got[5]) / 2.0;
  // N50: down the lengths, the first record at which twice the cumulative sum reaches sum_len; within a run of
  // `count` records of one length that is the j-th of them, j = ceil((sum_len - 2 cum) / (2 len))
  {
    std::vector<std::pair<int64_t, int64_t>> runs;
    walk_up(a, [&](int64_t len, int64_t count) { runs.emplace_back(len, count); });
    int64_t cum = 0, num = 0;
    for (size_t i = runs.size(); i-- > 0;) {
      const int64_t len = runs[i].first, count = runs[i].second;
      if (2 * (cum + len * count) >= a.sum_len) {
        const int64_t need = a.sum_len - 2 * cum;  // > 0 unless sum_len is 0
        const int64_t j = len > 0 ? std::max<int64_t>(1, (need + 2 * len - 1) / (2 * len)) : 1;
        o->n50 = len;
        o->n50_num = num + j;
        break;
      }
      cum += len * count;
      num += count;
    }
  }
  if (a.sum_len > 0) {  // a file of empty records: the ratios are 0
    const double s = (double)a.sum_len;
    o->q20_pct = 100.0 * (double)a.cnt[0] / s;
    o->q30_pct = 100.0 * (double)a.cnt[1] / s;
    o->gc_pct = 100.0 * (double)a.cnt[2] / s;
    if (a.ee > 0) o->avg_qual = 0.0 - 10.0 * log10(ldexp((double)a.ee, -kFxShift) / s);  // 0.0 - x: no "-0.00"
  }
}

std::string format_stat_table(const char* path, const StatAcc& a) {
  umiclust_fastq_stats t;
  finish_stats(a, &t);
  static const char* kNames[19] = {"file",    "format",  "type",   "num_seqs", "sum_len", "min_len", "avg_len",
                                   "max_len", "Q1",      "Q2",     "Q3",       "sum_gap", "N50",     "N50_num",
                                   "Q20(%)",  "Q30(%)",  "AvgQual", "GC(%)",   "sum_n"};
  static const char* kTypes[3] = {"DNA", "RNA", "Protein"};
  const std::string v[19] = {path ? path : "-",
                             "FASTQ",
                             kTypes[t.type],
                             commas((uint64_t)t.num_seqs),
                             commas((uint64_t)t.sum_len),
                             commas((uint64_t)t.min_len),
                             fixed(t.avg_len, 1, true),
                             commas((uint64_t)t.max_len),
                             fixed(t.q1, 1, true),
                             fixed(t.q2, 1, true),
                             fixed(t.q3, 1, true),
                             commas((uint64_t)t.sum_gap),
                             commas((uint64_t)t.n50),
                             commas((uint64_t)t.n50_num),
                             fixed(t.q20_pct, 2, false),
                             fixed(t.q30_pct, 2, false),
                             fixed(t.avg_qual, 2, false),
                             fixed(t.gc_pct, 2, false),
                             commas((uint64_t)t.sum_n)};
  std::string head, data;
  for (int k = 0; k < 19; k++) {
    const size_t w = std::max(strlen(kNames[k]), v[k].size());
    const std::string hp(w - strlen(kNames[k]), ' '), vp(w - v[k].size(), ' ');
    if (k) head += "  ", data += "  ";
    if (k < 3) {  // left-aligned
      head += kNames[k] + hp;
      data += v[k] + vp;
    } else {
      head += hp + kNames[k];
      data += vp + v[k];
    }
  }
  return head + "\n" + data + "\n";
}

// ------------------------------------------------------------------ the writers
namespace {

// writev of every piece (1024 at a time, partial writes resumed); a zero return with bytes left is an error
bool writev_all(int fd, std::vector<iovec>& iov) {
  size_t at = 0;
  while (at < iov.size()) {
    if (iov[at].iov_len == 0) {
      at++;
      continue;
    }
    const int n = (int)std::min<size_t>(iov.size() - at, 1024);
    const ssize_t w = writev(fd, iov.data() + at, n);
    if (w < 0) {
      if (errno == EINTR) continue;
      return false;
    }
    if (w == 0) return false;
    size_t left = (size_t)w;
    while (at < iov.size() && left >= iov[at].iov_len) left -= iov[at++].iov_len;
    if (left > 0) {
      iov[at].iov_base = (char*)iov[at].iov_base + left;
      iov[at].iov_len -= left;
    }
  }
  return true;
}

struct Out {
  int fd = -1;
  std::vector<iovec> iov;
  void add(const char* p, size_t n) {
    if (n == 0) return;
    if (!iov.empty() && (const char*)iov.back().iov_base + iov.back().iov_len == p) {
      iov.back().iov_len += n;  // neighbouring pieces of the mapping: one piece
      return;
    }
    iov.push_back({(void*)p, n});
  }
};

struct Chunk {
  std::vector<Rec> recs;
  std::vector<char> arena;
  Slot slot;
  int64_t qual_bytes = 0, begin = 0, next = 0;
  int rc = UMICLUST_OK;  // the indexer's (the records before a malformed one are in recs)
  std::string err;
  double t_read = 0.0;
  bool last = false;
};

}  // namespace

int64_t run_filter(const umiclust_fastq_filter_params& p, const Paths& paths, int threads, int64_t chunk_bytes,
                   Backend& be, umiclust_fastq_filter_result* res, std::string& err, const StatsReq* stats) {
  const double t_begin = now_s();
  umiclust_fastq_filter_result R;
  memset(&R, 0, sizeof(R));
  if (res) *res = R;
  const bool st = stats != nullptr;
  StatAcc acc_in, acc_kept;  // every record read, every record kept
  if (st && stats->before) memset(stats->before, 0, sizeof(*stats->before));
  if (st && stats->after) memset(stats->after, 0, sizeof(*stats->after));
  if (!paths.in) return err = "null input path", UMICLUST_EINVAL;
  if ((p.fastq_ascii != 33 && p.fastq_ascii != 64) || p.fastq_qmin < 0 || p.fastq_qmax < p.fastq_qmin ||
      p.fastq_minlen < 0 || std::isnan(p.fastq_maxee) || std::isnan(p.fastq_maxee_rate))
    return err = "bad fastq_filter parameters (fastq_ascii 33 or 64, 0 <= fastq_qmin <= fastq_qmax)", UMICLUST_EINVAL;
  threads = std::max(1, std::min(threads, 64));
  chunk_bytes = std::max(kChunkMin, chunk_bytes);
  Tables tab;
  build_tables(p.fastq_ascii, p.fastq_qmin, p.fastq_qmax, tab);

  // the input, mapped
  const int fd = open(paths.in, O_RDONLY);
  if (fd < 0) return err = std::string("cannot read ") + paths.in, UMICLUST_EIO;
  struct stat sb;
  if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
    close(fd);
    return err = std::string("cannot read ") + paths.in + " (not a regular file)", UMICLUST_EIO;
  }
  const int64_t size = (int64_t)sb.st_size;
  const char* data = nullptr;
  if (size > 0) {
    void* m = mmap(nullptr, (size_t)size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) {
      close(fd);
      return err = std::string("cannot map ") + paths.in, UMICLUST_EIO;
    }
    data = (const char*)m;
    (void)madvise(m, (size_t)size, MADV_SEQUENTIAL);
  }
  close(fd);
  auto unmap = [&] {
    if (data) munmap((void*)data, (size_t)size);
  };
  if (size >= 2 && (uint8_t)data[0] == 0x1f && (uint8_t)data[1] == 0x8b) {
    unmap();
    return err = std::string(paths.in) + " is gzip-compressed: only plain FASTQ is supported", UMICLUST_EINVAL;
  }
  Out outs[2];  // kept, discarded
  const char* opath[2] = {paths.out, paths.discarded};
  for (int k = 0; k < 2; k++)
    if (opath[k]) {
      outs[k].fd = open(opath[k], O_WRONLY | O_CREAT | O_TRUNC, 0666);
      if (outs[k].fd < 0) {
        if (k == 1 && outs[0].fd >= 0) close(outs[0].fd);
        unmap();
        return err = std::string("cannot write ") + opath[k], UMICLUST_EIO;
      }
    }

  // the pipeline: the parsing thread fills one chunk while the caller's thread runs the other through the backend,
  // the decision and the writers
  Chunk chunks[2];
  int state[2] = {0, 0};  // 0 free, 1 filled
  bool stop = false;
  std::mutex mu;
  std::condition_variable cv;
  std::thread producer([&] {
    int64_t pos = 0;
    bool multi_line = false;
    for (int64_t k = 0;; k++) {
      const int s = (int)(k & 1);
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return state[s] == 0 || stop; });
        if (stop) return;
      }
      Chunk& c = chunks[s];
      const double t0 = now_s();
      try {
        c.begin = pos;
        c.err.clear();
        c.rc = index_window(data, size, pos, pos + 2 * chunk_bytes, threads, c.recs, c.arena, &c.next, &multi_line, c.err);
        const int64_t n = (int64_t)c.recs.size();
        int64_t total = 0;
        for (const Rec& r : c.recs) total += r.len <= kDevMaxLen ? r.len : 0;
        c.qual_bytes = total;
        if (!be.reserve(s, (size_t)total, (size_t)n, st, c.slot, c.err)) {
          c.rc = UMICLUST_ENOMEM;
          c.recs.clear();
        } else {
          int64_t at = 0;
          for (int64_t i = 0; i < n; i++) {
            c.slot.offs[i] = at;
            at += c.recs[i].len <= kDevMaxLen ? c.recs[i].len : 0;
          }
          c.slot.offs[n] = at;
          memset(c.slot.qual, 0, (size_t)kPad);
          memset(c.slot.qual + kPad + total, 0, (size_t)kPad);
          if (st) {
            memset(c.slot.seq, 0, (size_t)kPad);
            memset(c.slot.seq + kPad + total, 0, (size_t)kPad);
          }
          const int T = (int)std::max<int64_t>(1, std::min<int64_t>(threads, n / 64));
          parallel_for(T, [&](int t) {
            for (int64_t i = n * t / T; i < n * (t + 1) / T; i++) {
              const Rec& r = c.recs[i];
              if (r.len > kDevMaxLen) continue;
              const char* from = r.arena ? c.arena.data() : data;
              memcpy(c.slot.qual + kPad + c.slot.offs[i], from + r.qual, (size_t)r.len);
              if (st) memcpy(c.slot.seq + kPad + c.slot.offs[i], from + r.seq, (size_t)r.len);
            }
          });
        }
      } catch (const std::bad_alloc&) {  // reported by the caller's thread
        c.rc = UMICLUST_ENOMEM;
        c.err.clear();
        c.recs.clear();
      }
      pos = c.next;
      c.last = c.rc != UMICLUST_OK || pos >= size;
      c.t_read = now_s() - t0;
      const bool last = c.last;
      {
        std::lock_guard<std::mutex> lk(mu);
        state[s] = 1;
      }
      cv.notify_all();
      if (last) return;
    }
  });

  int rc = UMICLUST_OK;
  static const char kAt = '@', kNl = '\n';
  static const char kPlus[] = "\n+\n";
  try {
    for (int64_t k = 0; size > 0; k++) {
      const int s = (int)(k & 1);
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return state[s] == 1; });
      }
      Chunk& c = chunks[s];
      const int64_t n = (int64_t)c.recs.size();
      R.t_read_s += c.t_read;
      if (c.rc == UMICLUST_ENOMEM) {
        rc = c.rc;
        err = c.err.empty() ? "host allocation failed" : c.err;
        break;
      }
      if (n > 0 || c.rc == UMICLUST_OK) R.n_chunks++;
      double t_h2d = 0.0, t_k = 0.0;
      if (n > 0 && !(st ? be.run_stats(s, (size_t)c.qual_bytes, n, tab.fx, p.fastq_ascii, &t_h2d, &t_k, err)
                        : be.run(s, (size_t)c.qual_bytes, n, tab.fx, &t_h2d, &t_k, err))) {
        rc = UMICLUST_EDEVICE;
        break;
      }
      R.t_h2d_s += t_h2d;
      R.t_kernel_s += t_k;
      const double tw0 = now_s();
      outs[0].iov.clear();
      outs[1].iov.clear();
      for (int64_t i = 0; i < n; i++) {
        const Rec& r = c.recs[i];
        const char* base = r.arena ? c.arena.data() : data;
        const uint8_t* q = (const uint8_t*)base + r.qual;
        const bool host_only = r.len > kDevMaxLen;
        int lo = 255, hi = 0;
        double ee;
        if (host_only) {
          unsigned __int128 acc = 0;
          for (int64_t j = 0; j < r.len; j++) {
            acc += tab.fx[q[j]];
            lo = std::min<int>(lo, q[j]);
            hi = std::max<int>(hi, q[j]);
          }
          ee = ldexp((double)acc, -kFxShift);
        } else {
          lo = c.slot.qlo[i];
          hi = c.slot.qhi[i];
          ee = ldexp((double)c.slot.ee[i], -kFxShift);
        }
        if (r.len > 0 && (lo < tab.lo || hi > tab.hi)) {  // O7b
          int64_t j = 0;
          while (j < r.len && q[j] >= tab.lo && q[j] <= tab.hi) j++;
          const int bad = j < r.len ? q[j] : 0;
          err = "FASTQ quality value (" + std::to_string(bad - p.fastq_ascii) + ") " +
                (bad < tab.lo ? "below qmin (" + std::to_string(p.fastq_qmin) : "above qmax (" + std::to_string(p.fastq_qmax)) +
                ") in record " + std::to_string(R.n_input) + " (" + std::string(data + r.label, (size_t)r.label_len) + ")";
          rc = UMICLUST_EFORMAT;
          break;
        }
        int why, band = 0;
        if (host_only) {
          why = decide_exact(p, tab, q, r.len);
        } else {
          why = decide_fx(p, r.len, c.slot.ee[i], &band);
          if (band) {
            why = decide_exact(p, tab, q, r.len);
            R.n_host_rechecked++;
          }
        }
        if (st) {  // the record's integers: the device's, or for a host-only record the same restatement's
          unsigned __int128 e128 = 0;
          uint64_t cnt[kCounts];
          if (host_only) {
            uint8_t l8, h8;
            record_stats((const uint8_t*)base + r.seq, q, r.len, tab.fx, p.fastq_ascii, &e128, &l8, &h8, cnt);
          } else {
            e128 = (unsigned __int128)(uint64_t)c.slot.ee[i];
            for (int j = 0; j < kCounts; j++) cnt[j] = c.slot.cnt[kCounts * i + j];
          }
          acc_in.add((const uint8_t*)base + r.seq, r.len, e128, cnt);
          if (why == 0) acc_kept.add((const uint8_t*)base + r.seq, r.len, e128, cnt);
        }
        R.n_input++;
        R.bases_in += r.len;
        R.ee_in += ee;
        if (why == 0) {
          R.n_kept++;
          R.bases_kept += r.len;
          R.ee_kept += ee;
        } else {
          R.n_discarded++;
          (why == 1 ? R.n_short : why == 2 ? R.n_long : why == 3 ? R.n_maxee : R.n_maxee_rate)++;
        }
        Out& o = outs[why == 0 ? 0 : 1];
        if (o.fd < 0) continue;
        if (r.verbatim) {
          o.add(data + r.begin, (size_t)(r.end - r.begin));
        } else {
          o.add(&kAt, 1);
          o.add(data + r.label, (size_t)r.label_len);
          o.add(&kNl, 1);
          o.add(base + r.seq, (size_t)r.len);
          o.add(kPlus, 3);
          o.add((const char*)q, (size_t)r.len);
          o.add(&kNl, 1);
        }
      }
      // both files at once
      bool wok[2] = {true, true};
      {
        std::thread side;
        if (outs[1].fd >= 0 && !outs[1].iov.empty()) side = std::thread([&] { wok[1] = writev_all(outs[1].fd, outs[1].iov); });
        if (outs[0].fd >= 0 && !outs[0].iov.empty()) wok[0] = writev_all(outs[0].fd, outs[0].iov);
        if (side.joinable()) side.join();
      }
      R.t_write_s += now_s() - tw0;
      if (!wok[0] || !wok[1]) {
        rc = UMICLUST_EIO;
        err = std::string("cannot write ") + opath[wok[0] ? 1 : 0];
        break;
      }
      if (rc != UMICLUST_OK) break;
      if (c.rc != UMICLUST_OK) {
        rc = c.rc;
        err = c.err;
        break;
      }
      // the chunk's pages of the input are not needed again
      {
        const int64_t pg = 4096, a = (c.begin + pg - 1) / pg * pg, b = c.next / pg * pg;
        if (b > a) (void)madvise((void*)(data + a), (size_t)(b - a), MADV_DONTNEED);
      }
      const bool last = c.last;
      {
        std::lock_guard<std::mutex> lk(mu);
        state[s] = 0;
      }
      cv.notify_all();
      if (last) break;
    }
  } catch (const std::bad_alloc&) {  // the parsing thread is still joined below
    rc = UMICLUST_ENOMEM;
    err = "host allocation failed";
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    stop = true;
  }
  cv.notify_all();
  producer.join();
  for (int k = 0; k < 2; k++)
    if (outs[k].fd >= 0 && close(outs[k].fd) != 0 && rc == UMICLUST_OK) {
      rc = UMICLUST_EIO;
      err = std::string("cannot write ") + opath[k];
    }
  unmap();
  R.t_total_s = now_s() - t_begin;
  if (res) *res = R;
  if (rc != UMICLUST_OK) return rc;
  if (paths.log) {
    char buf[1024];
    std::string log = "umiclust fastq_filter (drop-in for vsearch --fastq_filter)\n";
    log += std::string("input: ") + paths.in + "\n";
    snprintf(buf, sizeof(buf),
             "fastq_ascii %d, fastq_qmin %d, fastq_qmax %d, fastq_minlen %d, fastq_maxlen %d, fastq_maxee %g, "
             "fastq_maxee_rate %g (negative: not given)\n",
             p.fastq_ascii, p.fastq_qmin, p.fastq_qmax, p.fastq_minlen, p.fastq_maxlen, p.fastq_maxee,
             p.fastq_maxee_rate);
    log += buf;
    snprintf(buf, sizeof(buf), "%lld sequences kept (of which 0 truncated), %lld sequences discarded.\n",
             (long long)R.n_kept, (long long)R.n_discarded);
    log += buf;
    snprintf(buf, sizeof(buf),
             "discarded by first failing criterion: %lld fastq_minlen, %lld fastq_maxlen, %lld fastq_maxee, %lld "
             "fastq_maxee_rate\n%lld bases in, %lld bases kept; %lld records rechecked on the host; %lld chunks; %.3f s\n",
             (long long)R.n_short, (long long)R.n_long, (long long)R.n_maxee, (long long)R.n_maxee_rate,
             (long long)R.bases_in, (long long)R.bases_kept, (long long)R.n_host_rechecked, (long long)R.n_chunks,
             R.t_total_s);
    log += buf;
    const int lf = open(paths.log, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    bool ok = lf >= 0;
    if (ok) {
      std::vector<iovec> v{{(void*)log.data(), log.size()}};
      ok = writev_all(lf, v);
      ok = close(lf) == 0 && ok;
    }
    if (!ok) return err = std::string("cannot write ") + paths.log, UMICLUST_EIO;
  }
  if (st) {  // everything else succeeded: the two tables
    const char* txt[2] = {stats->before_txt, stats->after_txt};
    const char* file[2] = {paths.in, paths.out};
    const StatAcc* acc[2] = {&acc_in, &acc_kept};
    umiclust_fastq_stats* sout[2] = {stats->before, stats->after};
    for (int k = 0; k < 2; k++) {
      if (sout[k]) finish_stats(*acc[k], sout[k]);
      if (!txt[k]) continue;
      std::string table = format_stat_table(file[k], *acc[k]);
      const int tf = open(txt[k], O_WRONLY | O_CREAT | O_TRUNC, 0666);
      bool ok = tf >= 0;
      if (ok) {
        std::vector<iovec> v{{(void*)table.data(), table.size()}};
        ok = writev_all(tf, v);
        ok = close(tf) == 0 && ok;
      }
      if (!ok) return err = std::string("cannot write ") + txt[k], UMICLUST_EIO;
    }
  }
  return R.n_kept;
}

}  // namespace fq
}  // namespace uc

// ------------------------------------------------------------------ the argv grammar (O7e)
extern "C" int32_t umiclust_fastq_filter_params_from_argv(umiclust_fastq_filter_params* p, int32_t argc,
                                                          const char* const* argv, char* in_fastq, char* fastqout,
                                                          char* fastqout_discarded, char* log_path, int32_t pathcap) {
  if (!p || argc < 0 || (argc > 0 && !argv)) return UMICLUST_EINVAL;
  memset(p, 0, sizeof(*p));
  p->fastq_ascii = 33;
  p->fastq_qmin = 0;
  p->fastq_qmax = 41;
  p->fastq_minlen = 1;
  p->fastq_maxlen = -1;
  p->fastq_maxee = -1.0;
  p->fastq_maxee_rate = -1.0;
  char* bufs[4] = {in_fastq, fastqout, fastqout_discarded, log_path};
  for (char* b : bufs)
    if (b && pathcap > 0) b[0] = 0;
  bool have[4] = {false, false, false, false};
  auto set_path = [&](int k, const char* v) {
    have[k] = true;
    if (!bufs[k]) return true;
    if ((int64_t)strlen(v) >= pathcap) return false;
    strcpy(bufs[k], v);
    return true;
  };
  auto to_int = [](const char* v, int32_t* out) {
    char* e;
    errno = 0;
    const long x = strtol(v, &e, 10);
    if (e == v || *e || errno || x < INT32_MIN || x > INT32_MAX) return false;
    *out = (int32_t)x;
    return true;
  };
  auto to_dbl = [](const char* v, double* out) {
    char* e;
    errno = 0;
    const double x = strtod(v, &e);
    if (e == v || *e || errno || !(x >= 0.0)) return false;
    *out = x;
    return true;
  };
  int i = 0;
  if (argc > 0 && argv[0] && argv[0][0] != '-') i = 1;  // "vsearch"
  for (; i < argc; i++) {
    const char* a = argv[i];
    if (!a || a[0] != '-') return UMICLUST_EINVAL;
    const char* name = a[1] == '-' ? a + 2 : a + 1;
    if (!strcmp(name, "quiet") || !strcmp(name, "no_progress")) continue;
    if (i + 1 >= argc || !argv[i + 1]) return UMICLUST_EINVAL;
    const char* v = argv[++i];
    bool ok;
    int32_t ignored;
    if (!strcmp(name, "fastq_filter")) ok = set_path(0, v);
    else if (!strcmp(name, "fastqout")) ok = set_path(1, v);
    else if (!strcmp(name, "fastqout_discarded")) ok = set_path(2, v);
    else if (!strcmp(name, "log")) ok = set_path(3, v);
    else if (!strcmp(name, "fastq_ascii")) ok = to_int(v, &p->fastq_ascii) && (p->fastq_ascii == 33 || p->fastq_ascii == 64);
    else if (!strcmp(name, "fastq_qmin")) ok = to_int(v, &p->fastq_qmin);
    else if (!strcmp(name, "fastq_qmax")) ok = to_int(v, &p->fastq_qmax);
    else if (!strcmp(name, "fastq_minlen")) ok = to_int(v, &p->fastq_minlen) && p->fastq_minlen >= 0;
    else if (!strcmp(name, "fastq_maxlen")) ok = to_int(v, &p->fastq_maxlen) && p->fastq_maxlen >= 0;
    else if (!strcmp(name, "fastq_maxee")) ok = to_dbl(v, &p->fastq_maxee);
    else if (!strcmp(name, "fastq_maxee_rate")) ok = to_dbl(v, &p->fastq_maxee_rate);
    else if (!strcmp(name, "threads")) ok = to_int(v, &ignored);
    else ok = false;  // everything else, the truncation / strip / relabel / FASTA options included
    if (!ok) return UMICLUST_EINVAL;
  }
  if (!have[0] || (!have[1] && !have[2])) return UMICLUST_EINVAL;
  if (p->fastq_qmin < 0 || p->fastq_qmax < p->fastq_qmin) return UMICLUST_EINVAL;
  return UMICLUST_OK;
}
