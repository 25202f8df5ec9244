// deflate.h -- DEFLATE (RFC 1951) encoding of one BGZF block, HIP-free.
//
// Everything that decides a bit of the output is here, once, for the host and for the device: the tokeniser (one
// candidate per position from a hash table of last positions, verified byte by byte, greedy parse), the two histograms,
// the length-limited code builder, the code-length code with its run symbols, the exact bit counts of the three block
// forms and the choice among them, and the bit layout of header, tokens and end-of-block.  uc::dfl::run<Io> is the
// encoder on these pieces.  It is written for 64 lanes: a per-lane value is an Io::Lanes<T>, per-lane work is
// io.each([&](int lane) { ... }), and what an Io supplies is only how input bytes are fetched, how output words and
// bytes are put, and how the lanes combine what each saw (read of another lane's value, exclusive scan, the LDS
// max / add / or, uni() of a value all lanes share).  HostIo below is the serial restatement (each() loops over the 64 lanes, uc::deflate_block);
// bgzf.hip has the one that is a wave.  Everything outside each() is uniform over the lanes, and every combination of
// lane values is order-free (max, sum, or), so the host and the kernel produce the same bytes.
//
// The output is one deflate block with BFINAL = 1: stored, fixed or dynamic, whichever has the smallest exact bit
// count; on a tie stored wins over fixed and fixed over dynamic.  So the payload is never longer than the stored form,
// n + 5 bytes, and BSIZE always fits for n <= 0xff00.
#pragma once
#include <stdint.h>
#include <string.h>

#include "inflate.h"

// The encoder is serial, latency-bound code with many short loops; unrolled, the lead lane's loops cost the kernel 80
// spilled SGPRs and three times the VGPRs (make resources), so every loop of it stays a loop.
#if defined(__clang__)
#define UC_NO_UNROLL _Pragma("clang loop unroll(disable)")
#else
#define UC_NO_UNROLL
#endif

namespace uc {
namespace dfl {

constexpr uint32_t kMaxBlock = 0xff00;  // input bytes of one block
constexpr uint32_t kHashBits = 12, kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768;
enum : uint32_t { kStored = 0, kFixed = 1, kDynamic = 2 };
// what a block went through (Result::flags): the limiter ran on the literal/length, distance, code-length code; the
// distance set has no code, one code
enum : uint32_t { kLitLimited = 1, kDistLimited = 2, kClenLimited = 4, kDistNone = 8, kDistOne = 16 };

// a token: a literal byte, or kMatch | length << 16 | (distance - 1)
constexpr uint32_t kMatch = 1u << 31;

// the length symbol (0..28, + 257) of a match length 3..258 and the distance symbol (0..29) of a distance 1..32768:
// the inverses of inf::len_base / inf::dist_base, checked against them when this header is compiled
UC_HD constexpr uint32_t floor_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }
UC_HD constexpr uint32_t len_sym(uint32_t len) {
  const uint32_t x = len - 3;
  if (len == 258) return 28;
  if (x < 8) return x;
  const uint32_t e = floor_log2(x) - 2;
  return 4 * e + 4 + ((x >> e) & 3u);
}
UC_HD constexpr uint32_t dist_sym(uint32_t dist) {
  const uint32_t d = dist - 1;
  if (d < 4) return d;
  const uint32_t e = floor_log2(d) - 1;
  return 2 * e + 2 + ((d >> e) & 1u);
}
namespace spec {
constexpr bool symbols_match() {
  for (uint32_t i = 0; i < 29; i++) {
    const uint32_t lo = inf::len_base(i), hi = i == 28 ? 258 : lo + (1u << inf::len_extra(i)) - 1;
    if (len_sym(lo) != i || (len_sym(hi) != i && hi != 258)) return false;
  }
  for (uint32_t i = 0; i < 30; i++) {
    const uint32_t lo = inf::dist_base(i), hi = lo + (1u << inf::dist_extra(i)) - 1;
    if (dist_sym(lo) != i || dist_sym(hi) != i) return false;
  }
  return len_sym(257) == 27 && len_sym(258) == 28;
}
static_assert(symbols_match(), "len_sym / dist_sym are not the inverses of RFC 1951's tables");
}  // namespace spec

UC_HD inline uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }
UC_HD inline uint32_t clen_extra(uint32_t s) { return s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u; }

// The builder's scratch, and what outlives the hash table: every array that is indexed by a running value lives
// here (in LDS on the device), none on a lane's stack.
struct Build {
  uint32_t wt[288];    // weights of the internal nodes, in the order they are made (non-decreasing)
  uint16_t order[288]; // the used symbols by (count, symbol) ascending
  uint16_t par[288];   // an internal node's parent
  uint16_t depth[288];
  uint8_t nleaf[288];  // leaves directly under an internal node
  uint32_t cnt[16], next[16];
  uint32_t limited;
};
struct Codes {
  Build b;
  uint8_t lens[320];    // the dynamic code: literal/length lengths [0, hlit), distance lengths [hlit, hlit + hdist)
  uint8_t clen[20];     // the code-length code's lengths
  uint32_t chist[20];
  uint16_t citem[320];  // the code-length stream: symbol | extra value << 5
  uint16_t lcode[288], dcode[32], ccode[20];  // the codes that are emitted, bit-reversed
  uint8_t llen[288], dlen[32];
  uint32_t win[104];    // the staging window of emit_step: 31 carried bits + 64 x 48
  uint32_t hlit, hdist, hclen, nitem, kind, bits, flags;
};
// 17.7 KB: the hash table is dead once the block is tokenised, and the codes take its place
struct Work {
  union {
    uint32_t hash[1u << kHashBits];  // position + 1 of the last occurrence, 0 = none
    Codes c;
  };
  uint32_t lhist[288], dhist[32];
};
static_assert(sizeof(Codes) <= sizeof(uint32_t) << kHashBits, "the codes must fit where the hash table was");

struct Result {
  uint32_t kind, bytes, ntok, flags;
};

// Code lengths of at most `limit` bits for the symbols with hist[s] > 0: a pure function of hist.  Huffman's
// algorithm on the symbols sorted by (count, symbol) -- two queues, a leaf preferred on equal weight -- gives the
// number of codes per length; lengths past the limit are cut to it and the Kraft sum is brought back to 1 by
// lengthening the shortest-possible codes one at a time; the lengths then go to the symbols from the rarest (longest)
// to the most frequent.  One used symbol gets one bit (with min_codes == 2 a second, unused symbol gets the other, as
// the code-length code must be complete); none gives no code.  The result is complete whenever two or more symbols
// are used.  The rank sort is spread over the lanes; the rest is the lead lane's, between syncs.
// Bounds: rank 288 x 288 / 64; tree, depths and assignment <= 288 each; the limiter <= 288 x limit.
template <class Io>
UC_HD inline uint32_t build_lengths(Io& io, Build& B, const uint32_t* hist, int nsym, int limit, int min_codes,
                                    uint8_t* lens) {
  io.sync();
  io.each([&](int l) {
    UC_NO_UNROLL
    for (int s = l; s < nsym; s += 64) {
      lens[s] = 0;
      const uint32_t f = hist[s];
      if (!f) continue;
      int r = 0;
      UC_NO_UNROLL
      for (int t = 0; t < nsym; t++) {
        const uint32_t g = hist[t];
        r += (g && (g < f || (g == f && t < s))) ? 1 : 0;
      }
      B.order[r] = (uint16_t)s;
    }
  });
  io.sync();
  if (io.lead()) {
    int m = 0;
    UC_NO_UNROLL
    for (int s = 0; s < nsym; s++) m += hist[s] != 0;
    UC_NO_UNROLL
    for (int l = 0; l < 16; l++) B.cnt[l] = 0;
    B.limited = 0;
    if (m == 1) {
      lens[B.order[0]] = 1;
      if (min_codes > 1) lens[B.order[0] == 0 ? 1 : 0] = 1;
    } else if (m >= 2) {
      int li = 0, ii = 0;
      UC_NO_UNROLL
      for (int k = 0; k < m - 1; k++) {
        uint32_t w = 0, nl = 0;
        UC_NO_UNROLL
        for (int c = 0; c < 2; c++) {
          if (li < m && (ii >= k || hist[B.order[li]] <= B.wt[ii])) {
            w += hist[B.order[li++]];
            nl++;
          } else {
            w += B.wt[ii];
            B.par[ii++] = (uint16_t)k;
          }
        }
        B.wt[k] = w;
        B.nleaf[k] = (uint8_t)nl;
      }
      UC_NO_UNROLL
      for (int k = m - 2; k >= 0; k--) {
        const int d = k == m - 2 ? 0 : B.depth[B.par[k]] + 1;
        B.depth[k] = (uint16_t)d;
        if (d + 1 > limit && B.nleaf[k]) B.limited = 1;
        B.cnt[d + 1 > limit ? limit : d + 1] += B.nleaf[k];
      }
      if (B.limited) {
        uint32_t total = 0;
        UC_NO_UNROLL
        for (int l = 1; l <= limit; l++) total += B.cnt[l] << (limit - l);
        UC_NO_UNROLL
        for (int it = 0; it < 288 && total > (1u << limit); it++, total--) {
          B.cnt[limit]--;
          UC_NO_UNROLL
          for (int i = limit - 1; i >= 1; i--)
            if (B.cnt[i]) {
              B.cnt[i]--;
              B.cnt[i + 1] += 2;
              break;
            }
        }
      }
      int j = 0;
      UC_NO_UNROLL
      for (int l = limit; l >= 1; l--)
        UC_NO_UNROLL
        for (uint32_t c = 0; c < B.cnt[l] && j < m; c++) lens[B.order[j++]] = (uint8_t)l;
    }
  }
  io.sync();
  return io.uni(B.limited);
}

// the canonical code of lens[0 .. n), each code bit-reversed so that it goes to the stream lowest bit first
UC_HD inline void assign_codes(Build& B, const uint8_t* lens, int n, uint16_t* code) {
  UC_NO_UNROLL
  for (int l = 0; l < 16; l++) B.cnt[l] = 0;
  UC_NO_UNROLL
  for (int s = 0; s < n; s++) B.cnt[lens[s]]++;
  B.cnt[0] = 0;
  uint32_t c = 0;
  UC_NO_UNROLL
  for (int l = 1; l < 16; l++) {
    c = (c + B.cnt[l - 1]) << 1;
    B.next[l] = c;
  }
  UC_NO_UNROLL
  for (int s = 0; s < n; s++) code[s] = lens[s] ? (uint16_t)inf::bit_reverse(B.next[lens[s]]++, lens[s]) : (uint16_t)0;
}

// 64 items of at most 48 bits each (74 in all for the header step) appended at bit cursor `bitpos` of the output: a scan of the bit counts gives each
// lane its offset, the lanes OR their bits into the window, whose whole words then go out 64 adjacent words a store.
// The word the cursor ends in stays in win[0].  Every word stored lies wholly below the cursor.
template <class Io>
UC_HD inline void emit_step(Io& io, Codes& C, uint32_t& bitpos, typename Io::template Lanes<uint64_t>& bits,
                            typename Io::template Lanes<uint32_t>& nb) {
  uint32_t total = 0;
  typename Io::template Lanes<uint32_t> off = io.excl_scan(nb, total);
  const uint32_t r0 = bitpos & 31u, w0 = bitpos >> 5;
  io.each([&](int l) {
    const uint32_t n = nb[l];
    if (!n) return;
    const uint32_t o = r0 + off[l], w = o >> 5, s = o & 31u;
    const uint64_t v = bits[l];
    io.lds_or(&C.win[w], (uint32_t)(v << s));
    const uint64_t rest = v >> (32 - s);
    if (s + n > 32) io.lds_or(&C.win[w + 1], (uint32_t)rest);
    if (s + n > 64) io.lds_or(&C.win[w + 2], (uint32_t)(rest >> 32));
  });
  io.sync();
  const uint32_t full = (r0 + total) >> 5;
  const uint32_t partial = io.uni(C.win[full]);
  io.each([&](int l) {
    UC_NO_UNROLL
    for (uint32_t k = (uint32_t)l; k < full; k += 64) io.store32(w0 + k, C.win[k]);
  });
  io.sync();
  io.each([&](int l) {
    UC_NO_UNROLL
    for (uint32_t k = (uint32_t)l; k <= full; k += 64) C.win[k] = k ? 0u : partial;
  });
  io.sync();
  bitpos += total;
}

// One block of n <= kMaxBlock input bytes through io.
//
// Termination and bounds.  The tokeniser makes ceil(n / 64) steps; a step's compare loop makes at most 258 / 4 + 3
// iterations a lane, its parse at most 64; a position p is read only as p + k < n and a candidate lies before p.  There
// are at most n tokens (each covers at least one position), so the token store is n words.  The builder's loops are
// bounded by the alphabet sizes (above), the code-length stream has at most 316 items, the emit makes
// ceil((tokens + 1) / 64) steps.  The bytes put are [0, bytes) with bytes <= n + 5; an Io refuses a store past n + 5.
template <class Io>
UC_HD inline Result run(Io& io, Work& W, uint32_t n) {
  typedef typename Io::template Lanes<uint32_t> L32;
  typedef typename Io::template Lanes<uint64_t> L64;
  io.sync();
  io.each([&](int l) {
    UC_NO_UNROLL
    for (uint32_t k = (uint32_t)l; k < (1u << kHashBits); k += 64) W.hash[k] = 0;
    UC_NO_UNROLL
    for (uint32_t k = (uint32_t)l; k < 288; k += 64) W.lhist[k] = 0;
    if (l < 32) W.dhist[l] = 0;
  });
  io.sync();
  // ---- tokens and histograms
  uint32_t ntok = 0, carry = 0;  // carry: positions of this step that an earlier step's match covers
  UC_NO_UNROLL
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t cnt = n - base < 64 ? n - base : 64;
    L32 mlen, mdist, hv;
    io.each([&](int l) {
      const uint32_t p = base + (uint32_t)l;
      mlen[l] = 0, mdist[l] = 0, hv[l] = ~0u;
      if (p + kMinMatch > n) return;
      const uint32_t h = hash4(io.in4(p)), c = W.hash[h];
      hv[l] = h;
      if (!c || (uint32_t)l < carry || p - (c - 1) > kMaxDist) return;
      const uint32_t q = c - 1, maxl = n - p < kMaxMatch ? n - p : kMaxMatch;
      uint32_t k = 0;
      UC_NO_UNROLL
      while (k + 4 <= maxl) {
        const uint32_t x = io.in4(q + k) ^ io.in4(p + k);
        if (x) {
          k += (uint32_t)__builtin_ctz(x) >> 3;
          break;
        }
        k += 4;
      }
      if (k + 4 > maxl)
        UC_NO_UNROLL
        while (k < maxl && io.in(q + k) == io.in(p + k)) k++;
      if (k >= kMinMatch) mlen[l] = k, mdist[l] = p - q;
    });
    io.sync();  // every lookup of the step before any insert of it
    io.each([&](int l) {
      if (hv[l] != ~0u) io.lds_max(&W.hash[hv[l]], base + (uint32_t)l + 1);
    });
    uint64_t starts = 0;
    uint32_t i = carry;
    UC_NO_UNROLL
    while (i < cnt) {
      starts |= 1ull << i;
      const uint32_t len = io.read(mlen, i);
      i += len >= kMinMatch ? len : 1;
    }
    carry = i >= 64 ? i - 64 : 0;
    io.each([&](int l) {
      if (!((starts >> l) & 1)) return;
      const uint32_t t = ntok + (uint32_t)__builtin_popcountll(starts & ((1ull << l) - 1));
      if (mlen[l] >= kMinMatch) {
        io.tok_put(t, kMatch | mlen[l] << 16 | (mdist[l] - 1));
        io.lds_add(&W.lhist[257 + len_sym(mlen[l])], 1);
        io.lds_add(&W.dhist[dist_sym(mdist[l])], 1);
      } else {
        const uint32_t b = io.in(base + (uint32_t)l);
        io.tok_put(t, b);
        io.lds_add(&W.lhist[b], 1);
      }
    });
    ntok += (uint32_t)__builtin_popcountll(starts);
    io.sync();
  }
  if (io.lead()) W.lhist[256] = 1;
  io.sync();
  // ---- codes (the hash table is dead from here)
  Codes& C = W.c;
  uint32_t flags = 0;
  if (build_lengths(io, C.b, W.lhist, 286, 15, 1, C.lens)) flags |= kLitLimited;
  if (io.lead()) {
    uint32_t hlit = 286;
    UC_NO_UNROLL
    while (hlit > 257 && C.lens[hlit - 1] == 0) hlit--;
    C.hlit = hlit;
  }
  io.sync();
  const uint32_t hlit = io.uni(C.hlit);
  if (build_lengths(io, C.b, W.dhist, 30, 15, 1, C.lens + hlit)) flags |= kDistLimited;
  if (io.lead()) {
    uint32_t hdist = 30, used = 0;
    UC_NO_UNROLL
    for (int s = 0; s < 30; s++) used += W.dhist[s] != 0;
    UC_NO_UNROLL
    while (hdist > 1 && C.lens[hlit + hdist - 1] == 0) hdist--;
    C.hdist = hdist;
    C.flags = used == 0 ? (uint32_t)kDistNone : used == 1 ? (uint32_t)kDistOne : 0u;
    // the code-length stream
    UC_NO_UNROLL
    for (int s = 0; s < 20; s++) C.chist[s] = 0;
    const uint32_t tot = hlit + hdist;
    uint32_t ni = 0;
    auto item = [&](uint32_t s, uint32_t x) {
      C.citem[ni++] = (uint16_t)(s | x << 5);
      C.chist[s]++;
    };
    UC_NO_UNROLL
    for (uint32_t i = 0; i < tot;) {
      const uint32_t v = C.lens[i];
      uint32_t run = 1;
      UC_NO_UNROLL
      while (i + run < tot && C.lens[i + run] == v) run++;
      i += run;
      if (v == 0) {
        UC_NO_UNROLL
        while (run >= 11) {
          const uint32_t k = run < 138 ? run : 138;
          item(18, k - 11);
          run -= k;
        }
        if (run >= 3) item(17, run - 3), run = 0;
      } else {
        item(v, 0);
        run--;
        UC_NO_UNROLL
        while (run >= 3) {
          const uint32_t k = run < 6 ? run : 6;
          item(16, k - 3);
          run -= k;
        }
      }
      UC_NO_UNROLL
      for (; run; run--) item(v, 0);
    }
    C.nitem = ni;
  }
  if (build_lengths(io, C.b, C.chist, 19, 7, 2, C.clen)) flags |= kClenLimited;
  if (io.lead()) {
    uint32_t hclen = 19;
    UC_NO_UNROLL
    while (hclen > 4 && C.clen[inf::clen_order(hclen - 1)] == 0) hclen--;
    C.hclen = hclen;
    uint32_t extra = 0, dyn = 3 + 14 + 3 * hclen, fix = 3;
    UC_NO_UNROLL
    for (uint32_t s = 0; s < 19; s++) dyn += C.chist[s] * (C.clen[s] + clen_extra(s));
    UC_NO_UNROLL
    for (uint32_t s = 0; s < 286; s++) {
      const uint32_t f = W.lhist[s];
      dyn += f * (s < hlit ? C.lens[s] : 0u);
      fix += f * inf::fixed_lit_len(s);
      if (s > 256) extra += f * inf::len_extra(s - 257);
    }
    UC_NO_UNROLL
    for (uint32_t s = 0; s < 30; s++) {
      const uint32_t f = W.dhist[s];
      dyn += f * (s < C.hdist ? C.lens[hlit + s] : 0u);
      fix += f * 5;
      extra += f * inf::dist_extra(s);
    }
    dyn += extra, fix += extra;
    const uint32_t sto = 8 * (n + 5);
    C.kind = sto <= fix && sto <= dyn ? kStored : fix <= dyn ? kFixed : kDynamic;
    C.bits = C.kind == kStored ? sto : C.kind == kFixed ? fix : dyn;
    // the codes that are emitted
    if (C.kind == kFixed) {
      UC_NO_UNROLL
      for (uint32_t s = 0; s < 288; s++) C.llen[s] = (uint8_t)inf::fixed_lit_len(s);
      UC_NO_UNROLL
      for (uint32_t s = 0; s < 32; s++) C.dlen[s] = 5;
    } else {
      UC_NO_UNROLL
      for (uint32_t s = 0; s < 288; s++) C.llen[s] = s < hlit ? C.lens[s] : (uint8_t)0;
      UC_NO_UNROLL
      for (uint32_t s = 0; s < 32; s++) C.dlen[s] = s < C.hdist ? C.lens[hlit + s] : (uint8_t)0;
    }
    assign_codes(C.b, C.llen, 288, C.lcode);
    assign_codes(C.b, C.dlen, 32, C.dcode);
    assign_codes(C.b, C.clen, 19, C.ccode);
    UC_NO_UNROLL
    for (uint32_t k = 0; k < 104; k++) C.win[k] = 0;
  }
  io.sync();
  const uint32_t kind = io.uni(C.kind), nbits = io.uni(C.bits);
  Result R{kind, (nbits + 7) >> 3, ntok, flags | io.uni(C.flags)};
  // ---- emit
  if (kind == kStored) {
    io.each([&](int l) {
      UC_NO_UNROLL
      for (uint32_t k = (uint32_t)l; k < n + 5; k += 64) {
        const uint32_t v = k == 0 ? 1u : k == 1 ? n : k == 2 ? n >> 8 : k == 3 ? ~n : k == 4 ? ~n >> 8 : io.in(k - 5);
        io.store8(k, (uint8_t)v);
      }
    });
    io.sync();
    return R;
  }
  uint32_t bitpos = 0;
  L64 bits;
  L32 nb;
  const uint32_t hclen = io.uni(C.hclen), hdist = io.uni(C.hdist), nitem = io.uni(C.nitem);
  io.each([&](int l) {
    bits[l] = 0, nb[l] = 0;
    if (l == 0) {
      bits[l] = kind == kFixed ? 3u : 5u | (hlit - 257) << 3 | (hdist - 1) << 8 | (hclen - 4) << 13;
      nb[l] = kind == kFixed ? 3 : 17;
    } else if (kind == kDynamic && (uint32_t)l <= hclen) {
      bits[l] = C.clen[inf::clen_order((uint32_t)l - 1)];
      nb[l] = 3;
    }
  });
  emit_step(io, C, bitpos, bits, nb);
  if (kind == kDynamic)
    UC_NO_UNROLL
    for (uint32_t base = 0; base < nitem; base += 64) {
      io.each([&](int l) {
        bits[l] = 0, nb[l] = 0;
        if (base + (uint32_t)l >= nitem) return;
        const uint32_t it = C.citem[base + (uint32_t)l], s = it & 31u;
        bits[l] = (uint64_t)C.ccode[s] | (uint64_t)(it >> 5) << C.clen[s];
        nb[l] = C.clen[s] + clen_extra(s);
      });
      emit_step(io, C, bitpos, bits, nb);
    }
  UC_NO_UNROLL
  for (uint32_t base = 0; base <= ntok; base += 64) {  // the end-of-block symbol is item ntok
    io.each([&](int l) {
      const uint32_t t = base + (uint32_t)l;
      bits[l] = 0, nb[l] = 0;
      if (t > ntok) return;
      const uint32_t tok = t < ntok ? io.tok_get(t) : 256u;
      if (!(tok & kMatch)) {
        bits[l] = C.lcode[tok], nb[l] = C.llen[tok];
        return;
      }
      const uint32_t len = (tok >> 16) & 0x1ffu, dist = (tok & 0x7fffu) + 1, ls = len_sym(len), ds = dist_sym(dist);
      uint64_t v = C.lcode[257 + ls];
      uint32_t k = C.llen[257 + ls];
      v |= (uint64_t)(len - inf::len_base(ls)) << k, k += inf::len_extra(ls);
      v |= (uint64_t)C.dcode[ds] << k, k += C.dlen[ds];
      v |= (uint64_t)(dist - inf::dist_base(ds)) << k, k += inf::dist_extra(ds);
      bits[l] = v, nb[l] = k;
    });
    emit_step(io, C, bitpos, bits, nb);
  }
  // the bytes of the word the cursor stands in
  const uint32_t tail = ((bitpos & 31u) + 7) >> 3, last = io.uni(C.win[0]);
  io.each([&](int l) {
    if ((uint32_t)l < tail) io.store8((bitpos >> 5) * 4 + (uint32_t)l, (uint8_t)(last >> (8 * l)));
  });
  io.sync();
  if (bitpos != nbits) R.bytes = ~0u;  // the count and the emit disagree: the caller reports it
  return R;
}

// the serial Io: each() loops over the 64 lanes; no byte of `out` at or past cap = n + 5 is written
struct HostIo {
  template <class T>
  struct Lanes {
    T v[64];
    T& operator[](int l) { return v[l]; }
  };
  const uint8_t* src;
  uint8_t* out;
  uint32_t cap;
  uint32_t* tok;
  uint32_t tok_cap;
  int err;
  template <class F>
  void each(F f) {
    for (int l = 0; l < 64; l++) f(l);
  }
  bool lead() const { return true; }
  void sync() {}
  uint32_t uni(uint32_t v) const { return v; }  // a value that is the same on every lane
  uint32_t in(uint32_t p) const { return src[p]; }
  uint32_t in4(uint32_t p) const {
    uint32_t v;
    memcpy(&v, src + p, 4);
    return v;
  }
  uint32_t read(Lanes<uint32_t>& x, uint32_t i) { return x.v[i]; }
  Lanes<uint32_t> excl_scan(Lanes<uint32_t>& x, uint32_t& total) {
    Lanes<uint32_t> o;
    total = 0;
    for (int l = 0; l < 64; l++) o.v[l] = total, total += x.v[l];
    return o;
  }
  void lds_max(uint32_t* w, uint32_t v) { *w = *w < v ? v : *w; }
  void lds_add(uint32_t* w, uint32_t v) { *w += v; }
  void lds_or(uint32_t* w, uint32_t v) { *w |= v; }
  void tok_put(uint32_t i, uint32_t v) {
    if (i < tok_cap) tok[i] = v;
    else err = 1;
  }
  uint32_t tok_get(uint32_t i) const { return tok[i]; }
  void store32(uint32_t w, uint32_t v) {
    if (4 * w + 4 <= cap) memcpy(out + 4 * w, &v, 4);
    else err = 1;
  }
  void store8(uint32_t k, uint8_t v) {
    if (k < cap) out[k] = v;
    else err = 1;
  }
};

}  // namespace dfl

// The n <= 0xff00 bytes of src as one deflate block into out[0 .. n + 5): the host restatement of k_bgzf_deflate.
// tok: n words of scratch.  Returns false if the encoder contradicted itself (never seen; the caller falls back).
inline bool deflate_block(const uint8_t* src, uint32_t n, uint8_t* out, uint32_t* tok, dfl::Work& W, dfl::Result& R) {
  dfl::HostIo io{src, out, n + 5, tok, n, 0};
  R = dfl::run(io, W, n);
  return !io.err && R.bytes <= n + 5;
}

}  // namespace uc
