// inflate.h -- DEFLATE (RFC 1951) decoding of one BGZF block, HIP-free.
//
// Everything that decides whether a stream is accepted is here, once, for the host and for the device: the block
// header, the stored block's LEN/NLEN check, the HLIT/HDIST limits, the code-length code with its repeat codes, the
// canonical-code construction under zlib's rules (inflate_table), the length / distance tables and the fixed code.
// uc::inf::run<Io> is the decoder on these pieces; what an Io supplies is only how bits are fetched and how bytes are
// put: HostIo below is the plain serial one (uc::inflate_block, the host restatement of k_bgzf_inflate, as
// bam::scan_record restates k_bam_scan), bgzf.hip has the one whose 64 lanes work together.  Every decision in run<>
// is uniform over the lanes of an Io; lane() / lanes() / sync() only spread table filling.
//
// Accepted exactly when zlib's inflate accepts under the host reader's rule (io::inflate_bgzf): the final block's end
// is reached with exactly isize bytes out; input left over is ignored; CRC32 is not looked at.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define UC_HD __host__ __device__
#else
#define UC_HD
#endif

namespace uc {
namespace inf {

// the per-block status: 0 = ok, > 0 = the error class
enum : int32_t {
  kOk = 0,
  kEInput = 1,        // the payload ends inside the stream
  kEBlockType = 2,    // BTYPE 3
  kEStored = 3,       // LEN != ~NLEN
  kECounts = 4,       // HLIT > 286 or HDIST > 30
  kECodeLengths = 5,  // repeat with no previous length, or a run past HLIT + HDIST
  kECodeSet = 6,      // over-subscribed or incomplete code, or no code for symbol 256
  kESymbol = 7,       // a bit pattern no code has, or a literal/length symbol >= 286, a distance symbol >= 30
  kEDistance = 8,     // a distance past the bytes written so far in this block
  kEOutput = 9,       // more than isize bytes
  kEShort = 10,       // the final block ends before isize bytes
};
constexpr int kNumStatus = 11;
inline const char* status_name(int32_t s) {
  static const char* const names[kNumStatus] = {"ok", "input ends inside the stream", "reserved block type",
      "stored length check", "too many length or distance codes", "bad code-length repeat", "bad code set",
      "invalid code", "distance too far back", "more than ISIZE bytes", "fewer than ISIZE bytes"};
  return s >= 0 && s < kNumStatus ? names[s] : "unknown";
}

// A canonical code: count[l] = codes of length l, sym[] = the symbols in code order, tab[] = the primary table on the
// low kBits stream bits (symbol << 4 | length; 0 = no code of at most kBits bits has these bits: the overflow walk).
template <int kBits_, int kSyms_>
struct Huff {
  static constexpr int kBits = kBits_, kSyms = kSyms_;
  uint16_t count[16];
  uint16_t offs[16];
  uint16_t sym[kSyms_];
  uint16_t tab[1 << kBits_];
};
// The tables of one deflate block: 3.6 KB.  The code-length code (19 symbols) is built in `dist` before the distance
// code takes its place.
struct Tables {
  Huff<10, 288> lit;
  Huff<8, 32> dist;
  uint8_t lens[320];
};

// The length and distance tables of RFC 1951 §3.2.5.  The decoder sits on a serial chain per symbol, so base and
// extra bits are computed from the symbol (no memory load); the tables themselves stand below as the specification,
// and the arithmetic is checked against every entry of them when this header is compiled.
UC_HD constexpr uint32_t len_extra(uint32_t i) { return i < 8 || i == 28 ? 0u : (i - 4) >> 2; }
UC_HD constexpr uint32_t len_base(uint32_t i) { return i < 8 ? 3 + i : i == 28 ? 258u : 3 + ((4 + (i & 3)) << len_extra(i)); }
UC_HD constexpr uint32_t dist_extra(uint32_t i) { return i < 4 ? 0u : (i - 2) >> 1; }
UC_HD constexpr uint32_t dist_base(uint32_t i) { return i < 4 ? 1 + i : 1 + ((2 + (i & 1)) << dist_extra(i)); }
namespace spec {
constexpr uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99,
                                   115, 131, 163, 195, 227, 258};
constexpr uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025,
                                    1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12,
                                    12, 13, 13};
constexpr bool tables_match() {
  for (uint32_t i = 0; i < 29; i++)
    if (len_base(i) != kLenBase[i] || len_extra(i) != kLenExtra[i]) return false;
  for (uint32_t i = 0; i < 30; i++)
    if (dist_base(i) != kDistBase[i] || dist_extra(i) != kDistExtra[i]) return false;
  return true;
}
static_assert(tables_match(), "len_base / len_extra / dist_base / dist_extra differ from RFC 1951's tables");
}  // namespace spec
UC_HD inline uint32_t clen_order(uint32_t i) {
  constexpr uint8_t t[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return t[i];
}
// the fixed code's length of literal/length symbol s (288 symbols) -- its distance code is 32 symbols of 5 bits
UC_HD inline uint32_t fixed_lit_len(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

UC_HD inline uint32_t bit_reverse(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; i++) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}

// The canonical code of lens[0 .. n) into h, under inflate_table's rules: an over-subscribed set is refused; an
// incomplete one is refused unless `single_ok` and its longest code has 1 bit; a set without any code is accepted
// (its every bit pattern then fails in huff_decode).  count / offs / sym are written by lane 0 alone, between
// syncs, and read by all; the primary table is cleared and filled lane-strided.  Returns kOk or kECodeSet, the same
// on every lane.
template <class H, class Io>
UC_HD inline int32_t huff_build(H& h, const uint8_t* lens, int n, bool single_ok, Io& io) {
  io.sync();  // the previous table's readers and the writer of lens are done
  if (io.lane() == 0) {
    for (int l = 0; l < 16; l++) h.count[l] = 0;
    for (int s = 0; s < n; s++) h.count[lens[s]]++;
  }
  io.sync();
  int left = 1, longest = 0;
  for (int l = 1; l < 16; l++) {
    left = (left << 1) - (int)h.count[l];
    if (left < 0) return kECodeSet;
    if (h.count[l]) longest = l;
  }
  if (longest && left > 0 && !(single_ok && longest == 1)) return kECodeSet;
  if (io.lane() == 0) {
    h.offs[1] = 0;
    for (int l = 1; l < 15; l++) h.offs[l + 1] = (uint16_t)(h.offs[l] + h.count[l]);
    for (int s = 0; s < n; s++)
      if (lens[s]) h.sym[h.offs[lens[s]]++] = (uint16_t)s;
  }
  for (int i = io.lane(); i < (1 << H::kBits); i += io.lanes()) h.tab[i] = 0;
  io.sync();
  const int coded = n - (int)h.count[0];
  for (int i = io.lane(); i < coded; i += io.lanes()) {
    // the i-th symbol in code order: its length l and its code
    int idx = 0, l = 1;
    uint32_t first = 0;
    for (; l < 16; l++) {
      const int c = h.count[l];
      if (i < idx + c) break;
      idx += c;
      first = (first + (uint32_t)c) << 1;
    }
    if (l > H::kBits) continue;
    const uint16_t e = (uint16_t)((uint32_t)h.sym[i] << 4 | (uint32_t)l);
    for (uint32_t j = bit_reverse(first + (uint32_t)(i - idx), l); j < (1u << H::kBits); j += 1u << l) h.tab[j] = e;
  }
  io.sync();
  return kOk;
}

// The symbol whose code starts the stream bits `b` (at least 15 of them, the first bit lowest), its length in len;
// -1 where no code of h matches.
template <class H>
UC_HD inline int huff_decode(const H& h, uint32_t b, int& len) {
  const uint32_t e = h.tab[b & ((1u << H::kBits) - 1)];
  if (e) {
    len = (int)(e & 15u);
    return (int)(e >> 4);
  }
  // the overflow walk: one bit at a time in code order (at most 15 steps)
  int code = 0, first = 0, index = 0;
  for (int l = 1; l < 16; l++) {
    code |= (int)((b >> (l - 1)) & 1u);
    const int c = h.count[l];
    if (code - c < first) {
      len = l;
      return h.sym[index + (code - first)];
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1;
}

// The code lengths of a dynamic block into T.lens[0 .. nlen + ndist), through the code-length code built in T.dist.
// T.lens is written by lane 0 alone; nothing here reads it back before a sync.
template <class Io>
UC_HD inline int32_t read_dynamic_lens(Io& io, Tables& T, int& nlen, int& ndist) {
  const uint32_t hdr = io.peek();
  if (!io.consume(14)) return kEInput;
  nlen = (int)(hdr & 31u) + 257;
  ndist = (int)((hdr >> 5) & 31u) + 1;
  const int ncode = (int)((hdr >> 10) & 15u) + 4;
  if (nlen > 286 || ndist > 30) return kECounts;
  io.sync();
  for (int i = io.lane(); i < 19; i += io.lanes()) T.lens[i] = 0;
  io.sync();
  for (int i = 0; i < ncode; i++) {
    const uint32_t b = io.peek();
    if (!io.consume(3)) return kEInput;
    if (io.lane() == 0) T.lens[clen_order((uint32_t)i)] = (uint8_t)(b & 7u);
  }
  if (const int32_t rc = huff_build(T.dist, T.lens, 19, false, io)) return rc;
  // every step consumes at least one bit (a code of the code-length code) or fails
  int have = 0;
  uint32_t prev = 0;
  while (have < nlen + ndist) {
    int l = 0;
    const int s = huff_decode(T.dist, io.peek(), l);
    if (s < 0) return kESymbol;
    if (!io.consume((uint32_t)l)) return kEInput;
    if (s < 16) {
      if (io.lane() == 0) T.lens[have] = (uint8_t)s;
      have++;
      prev = (uint32_t)s;
      continue;
    }
    const uint32_t eb = s == 16 ? 2u : s == 17 ? 3u : 7u;
    const uint32_t x = io.peek() & ((1u << eb) - 1u);
    if (!io.consume(eb)) return kEInput;
    if (s == 16 && have == 0) return kECodeLengths;
    const int rep = (int)x + (s == 18 ? 11 : 3);
    const uint8_t v = s == 16 ? (uint8_t)prev : (uint8_t)0;
    if (s != 16) prev = 0;
    if (have + rep > nlen + ndist) return kECodeLengths;
    if (io.lane() == 0)
      for (int i = 0; i < rep; i++) T.lens[have + i] = v;
    have += rep;
  }
  io.sync();
  if (T.lens[256] == 0) return kECodeSet;
  return kOk;
}

// One BGZF block's DEFLATE stream through io into isize bytes.
//
// Termination and bounds.  io.consume(n) fails, without advancing, once the cursor would pass the payload's last bit,
// so what is consumed in all is bounded by the payload's length.  Every iteration of the block loop consumes the 3
// header bits or fails; every iteration of the symbol loop consumes at least the 1 bit of a literal/length code or
// fails; read_dynamic_lens likewise.  A byte is put only at out < isize (literal), out + len <= isize (match and
// stored, in the form len <= isize - out, which cannot wrap), and a match reads only [out - dist, out) with
// dist <= out: nothing before the block's first byte, BGZF blocks having no preset dictionary.
template <class Io>
UC_HD inline int32_t run(Io& io, Tables& T, uint32_t isize) {
  uint32_t out = 0;
  for (;;) {
    const uint32_t hdr = io.peek();
    if (!io.consume(3)) return kEInput;
    const bool last = hdr & 1u;
    const uint32_t type = (hdr >> 1) & 3u;
    if (type == 3) return kEBlockType;
    if (type == 0) {
      io.align_byte();
      const uint32_t v = io.peek();
      if (!io.consume(32)) return kEInput;
      const uint32_t len = v & 0xffffu;
      if (len != (~(v >> 16) & 0xffffu)) return kEStored;
      if (len > io.bytes_left()) return kEInput;
      if (len > isize - out) return kEOutput;
      io.stored(out, len);
      out += len;
    } else {
      int nlen = 288, ndist = 32;
      if (type == 1) {
        io.sync();
        for (int i = io.lane(); i < 320; i += io.lanes()) T.lens[i] = i < 288 ? (uint8_t)fixed_lit_len((uint32_t)i) : 5;
        io.sync();
      } else if (const int32_t rc = read_dynamic_lens(io, T, nlen, ndist)) {
        return rc;
      }
      if (const int32_t rc = huff_build(T.lit, T.lens, nlen, true, io)) return rc;
      if (const int32_t rc = huff_build(T.dist, T.lens + nlen, ndist, true, io)) return rc;
      for (;;) {
        int l = 0;
        int s = huff_decode(T.lit, io.peek(), l);
        if (s < 0) return kESymbol;
        if (!io.consume((uint32_t)l)) return kEInput;
        if (s < 256) {
          if (out >= isize) return kEOutput;
          io.literal(out, (uint8_t)s);
          out++;
          continue;
        }
        if (s == 256) break;
        s -= 257;
        if (s >= 29) return kESymbol;
        uint32_t eb = len_extra((uint32_t)s);
        const uint32_t len = len_base((uint32_t)s) + (io.peek() & ((1u << eb) - 1u));
        if (!io.consume(eb)) return kEInput;
        const int d = huff_decode(T.dist, io.peek(), l);
        if (d < 0 || d >= 30) return kESymbol;
        if (!io.consume((uint32_t)l)) return kEInput;
        eb = dist_extra((uint32_t)d);
        const uint32_t dist = dist_base((uint32_t)d) + (io.peek() & ((1u << eb) - 1u));
        if (!io.consume(eb)) return kEInput;
        if (dist > out) return kEDistance;
        if (len > isize - out) return kEOutput;
        io.match(out, len, dist);
        out += len;
      }
    }
    if (last) break;
  }
  io.finish(out);
  return out == isize ? kOk : kEShort;
}

// the serial Io: no byte of `in` past in_len is read, no byte of `out` past what run<> allows is written
struct HostIo {
  const uint8_t* in;
  uint64_t pos, end;  // in bits
  uint8_t* out;
  int lane() const { return 0; }
  int lanes() const { return 1; }
  void sync() {}
  // the next 32 stream bits, the first one lowest; zero past the payload's end (consume refuses those)
  uint32_t peek() const {
    uint64_t v = 0;
    const uint64_t byte = pos >> 3;
    for (uint64_t i = 0; i < 5; i++)
      if ((byte + i) * 8 < end) v |= (uint64_t)in[byte + i] << (8 * i);
    return (uint32_t)(v >> (pos & 7));
  }
  bool consume(uint32_t n) {
    if (pos + n > end) return false;
    pos += n;
    return true;
  }
  void align_byte() { pos = (pos + 7) & ~(uint64_t)7; }
  uint32_t bytes_left() const { return (uint32_t)((end - pos) >> 3); }
  void literal(uint32_t o, uint8_t c) { out[o] = c; }
  void stored(uint32_t o, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) out[o + i] = in[(pos >> 3) + i];
    pos += (uint64_t)len * 8;
  }
  void match(uint32_t o, uint32_t len, uint32_t dist) {
    for (uint32_t i = 0; i < len; i++) out[o + i] = out[o + i - dist];
  }
  void finish(uint32_t) {}
};

}  // namespace inf

// The DEFLATE stream in[0 .. in_len) of one BGZF block into out[0 .. isize): an inf:: status.
inline int32_t inflate_block(const uint8_t* in, uint32_t in_len, uint8_t* out, uint32_t isize) {
  inf::Tables T;
  inf::HostIo io{in, 0, (uint64_t)in_len * 8, out};
  return inf::run(io, T, isize);
}

}  // namespace uc
