// dropin_extract.cpp -- UMI extraction (§8f f1): the host side of csrc/extract.hip on the context core (ctx.h).
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"

using namespace uc;
using namespace uc::io;

namespace {
// additionalEqualities of extract_umis.py:26-87 (either order), plus identity
constexpr const char* kIupacEq[] = {"MA", "MC", "RA", "RG", "WA", "WT", "SC", "SG", "YC", "YT", "KG", "KT", "VA", "VC",
                                "VG", "HA", "HC", "HT", "DA", "DG", "DT", "BC", "BG", "BT", "NA", "NC", "NG", "NT",
                                "ma", "mc", "ra", "rg", "wa", "wt", "sc", "sg", "yc", "yt", "kg", "kt", "va", "vc",
                                "vg", "ha", "hc", "ht", "da", "dg", "dt", "bc", "bg", "bt", "na", "nc", "ng", "nt",
                                "aA", "cC", "tT", "gG"};

// symbol equality of edlib with the reference's additionalEqualities, built at compile time (constant
// initialisation: contexts on different threads share it without a lazy first-use race)
struct EqTable {
  bool eq[256][256];
};
constexpr EqTable make_eq_table() {
  EqTable t{};
  for (int a = 0; a < 256; a++)
    for (int b = 0; b < 256; b++) t.eq[a][b] = a == b;
  for (const char* e : kIupacEq) {
    t.eq[(uint8_t)e[0]][(uint8_t)e[1]] = true;
    t.eq[(uint8_t)e[1]][(uint8_t)e[0]] = true;
  }
  return t;
}
constexpr EqTable kEqTable = make_eq_table();
}  // namespace

void uc::build_patterns(Ctx* c, const char* fwd, const char* rev, ExtractPatterns& P) {
  const auto& eqt = kEqTable.eq;
  memset(&P, 0, sizeof(P));
  const char* pats[2] = {fwd, rev};
  for (int w = 0; w < 2; w++) {
    if (!pats[w]) c->fail(UMICLUST_EINVAL, "null pattern");
    const int m = (int)strlen(pats[w]);
    if (m < 1 || m > 64) c->fail(UMICLUST_EINVAL, "UMI patterns of 1..64 symbols are supported (got %d)", m);
    P.m[w] = m;
    for (int ch = 0; ch < 256; ch++)
      for (int i = 0; i < m; i++) {
        if (eqt[(uint8_t)pats[w][i]][ch]) P.peq[w][ch] |= 1ull << i;
        if (eqt[(uint8_t)pats[w][m - 1 - i]][ch]) P.peqr[w][ch] |= 1ull << i;
      }
  }
}

namespace {
void extract_device(Ctx* c, const char* seqs, const int64_t* offs, int64_t n, int32_t a5, int32_t a3,
                    int32_t k, const char* fwd, const char* rev, int32_t* out) {
  if (n < 0 || (n > 0 && (!seqs || !offs || !out)) || a5 < 0 || a3 < 0 || k < 0)
    c->fail(UMICLUST_EINVAL, "bad argument");
  ExtractPatterns P;
  build_patterns(c, fwd, rev, P);
  if (n == 0) return;
  // Only the adapter windows are read: with short windows the host gathers them (its threads, into pinned
  // memory) and the device gets ~141 B per read instead of the whole read
  const int32_t S = (a5 + a3 + 3) & ~3;
  if (a3 > 0 && a5 + a3 > 0 && S <= kExMaxSlot && a5 <= 255 && a3 <= 255) {
    ExtractState& X = c->ex;
    c->hip(X.win.ensure((size_t)n * S + 16), "alloc pinned");
    c->hip(X.len.ensure((size_t)n * 2), "alloc pinned");
    const int T = n < 65536 ? 1 : io_threads();
    parallel_for(T, [&](int t) {
      const int64_t lo = n * t / T, hi = n * (t + 1) / T;
      for (int64_t i = lo; i < hi; i++) {
        const char* b = seqs + offs[i];
        const int64_t len = offs[i + 1] - offs[i];
        // Python slicing: seq[:a5] and seq[-a3:]
        const int64_t l5 = a5 < len ? a5 : len, l3 = a3 < len ? a3 : len;
        char* d = X.win.p + i * S;
        memcpy(d, b, (size_t)l5);
        memcpy(d + a5, b + len - l3, (size_t)l3);
        X.len.p[2 * i] = (uint8_t)l5;
        X.len.p[2 * i + 1] = (uint8_t)l3;
      }
    });
    c->hip(X.dwin.ensure((size_t)n * S + 16), "alloc");
    c->hip(X.dlen.ensure((size_t)n * 2), "alloc");
    c->hip(X.dout.ensure((size_t)n * 6), "alloc");
    c->hip(X.dpat.ensure(1), "alloc");
    c->hip(hipMemcpyAsync(X.dwin.p, X.win.p, (size_t)n * S, hipMemcpyHostToDevice, c->st), "h2d");
    c->hip(hipMemcpyAsync(X.dlen.p, X.len.p, (size_t)n * 2, hipMemcpyHostToDevice, c->st), "h2d");
    c->hip(hipMemcpyAsync(X.dpat.p, &P, sizeof(P), hipMemcpyHostToDevice, c->st), "h2d");
    c->hip(launch_extract_win(X.dwin.p, X.dlen.p, n, S, a5, k, X.dpat.p, X.dout.p, c->st), "extract");
    c->hip(hipMemcpyAsync(out, X.dout.p, (size_t)n * 6 * 4, hipMemcpyDeviceToHost, c->st), "d2h");
    c->hip(hipStreamSynchronize(c->st), "sync");
    return;
  }
  std::vector<int64_t> rel;
  DevBuf<char> d_s;
  DevBuf<int64_t> d_o;
  DevBuf<ExtractPatterns> d_p;
  DevBuf<int32_t> d_out;
  c->hip(d_p.ensure(1), "alloc");
  c->hip(d_out.ensure((size_t)n * 6), "alloc");
  upload_seqs(c, seqs, offs, n, d_s, d_o, rel, c->st);
  c->hip(hipMemcpyAsync(d_p.p, &P, sizeof(P), hipMemcpyHostToDevice, c->st), "h2d");
  c->hip(launch_extract(d_s.p, d_o.p, n, a5, a3, k, d_p.p, d_out.p, c->st), "extract");
  c->hip(hipMemcpyAsync(out, d_out.p, (size_t)n * 6 * 4, hipMemcpyDeviceToHost, c->st), "d2h");
  c->hip(hipStreamSynchronize(c->st), "sync");
}

}  // namespace

int32_t umiclust_extract_umis(umiclust_ctx* ctx, const char* seqs, const int64_t* offsets, int64_t n,
                              int32_t adapter_length_5_end, int32_t adapter_length_3_end, int32_t max_pattern_dist,
                              const char* umi_fwd, const char* umi_rev, int32_t* out) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    extract_device(c, seqs, offsets, n, adapter_length_5_end, adapter_length_3_end, max_pattern_dist, umi_fwd,
                   umi_rev, out);
    return UMICLUST_OK;
  });
}

int64_t umiclust_extract_umis_file(umiclust_ctx* ctx, const char* fastx_file, const char* out_fasta,
                                   int32_t adapter_length_5_end, int32_t adapter_length_3_end,
                                   int32_t max_pattern_dist, const char* umi_fwd, const char* umi_rev) {
  uc::Ctx* c = uc::core(ctx);
  UC_GUARD(c, {
    if (!fastx_file || !out_fasta) c->fail(UMICLUST_EINVAL, "null path");
    Fasta f;
    bool fastq = false;
    {
      FILE* fp = fopen(fastx_file, "rb");
      if (!fp) c->fail(UMICLUST_EIO, "cannot read %s", fastx_file);
      int ch;
      while ((ch = fgetc(fp)) == '\n' || ch == '\r') {}
      fastq = ch == '@';
      fclose(fp);
    }
    if (!(fastq ? io::read_fastq(fastx_file, f) : io::read_fasta(fastx_file, f)))
      c->fail(UMICLUST_EIO, "cannot parse %s", fastx_file);
    const int64_t n = (int64_t)f.hdr_off.size();
    std::vector<int32_t> res((size_t)std::max<int64_t>(n, 1) * 6);
    extract_device(c, f.seq.data(), f.seq_off.data(), n, adapter_length_5_end, adapter_length_3_end, max_pattern_dist,
                   umi_fwd, umi_rev, res.data());
    // records in input order; the reference raises at the first record without a strand annotation, after
    // writing the records before it: those are written, then the error is returned
    int64_t ngood = n;
    for (int64_t i = 0; i < n && ngood == n; i++) {
      Sv st;
      if (!split1(Sv{f.data + f.hdr_off[i], (size_t)f.hdr_len[i]}, "strand=", st)) ngood = i;
    }
    const int64_t tot = io::write_detected_umis(out_fasta, f, res.data(), ngood, adapter_length_3_end);
    if (ngood < n) c->fail(UMICLUST_EFORMAT, "Read strand not annotated!");
    return tot;
  });
}
