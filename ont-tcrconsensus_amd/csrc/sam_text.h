// sam_text.h -- SAM text to BAM records, HIP-free (policy O9: restated, not pinned).
//
// Everything that decides what a SAM line becomes is here, once, for the host and for the device: the field split, the
// number formats, the CIGAR and aux rules and the sort key (the record layout and reg2bin: bam_record.h).  sam::measure<Io>
// sizes a line and sam::encode<Io> writes its record; what an Io supplies is only how text bytes are fetched, how record
// bytes are put and how the lanes of an Io add up what each of them saw: HostIo below is the plain serial one
// (sam::encode_host, the host restatement of the kernels of samsort.hip, as uc::inflate_block restates k_bgzf_inflate),
// samsort.hip has the one whose 64 lanes work together.  Every decision is the same on all lanes of an Io.
//
// The rules restate htslib's sam_parse1 and samtools' coordinate order (bam1_cmp_core under SO:coordinate, ties in
// input order).  Where this file is stricter than htslib it refuses, which is louder than guessing:
//   - numbers are plain decimal digits, at most 10 of them (aux i: an optional '-' in front), no sign on FLAG, POS,
//     MAPQ, PNEXT, no hex; a CIGAR length has at most 9 digits;
//   - none of the 11 mandatory fields may be empty;
//   - aux types B and anything outside A i f Z H are refused; a CIGAR of more than 65535 ops is refused (the CG-tag
//     form is not written);
//   - the flag is stored as it stands: htslib's "mapped query without a coordinate becomes unmapped" edit is not made.
// A '\r' is data like any other byte: a file with CR LF line ends has a '\r' at the end of its last field, which a
// QUAL, an aux Z value or a header field then holds (and a number refuses).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_set>
#include <vector>

#include "bam_record.h"  // the record's layout, reg2bin, mix64, and UC_HD

namespace uc {
namespace sam {

// a line's status: code | field << 8; code 0 = ok
enum : int32_t { kOk = 0, kEFormat = 1, kERange = 2 };
// field 0 = the line itself (empty, or fewer than 11 fields), 1..11 = the mandatory fields, 12 = an aux field
enum : int32_t { kFLine = 0, kFQname = 1, kFFlag, kFRname, kFPos, kFMapq, kFCigar, kFRnext, kFPnext, kFTlen, kFSeq,
                 kFQual, kFAux };
UC_HD inline int32_t bad(int32_t code, int32_t field) { return code | (field << 8); }
inline const char* field_name(int32_t f) {
  static const char* const names[13] = {"line", "QNAME", "FLAG", "RNAME", "POS", "MAPQ", "CIGAR", "RNEXT", "PNEXT",
                                        "TLEN", "SEQ", "QUAL", "aux"};
  return f >= 0 && f < 13 ? names[f] : "?";
}

constexpr int64_t kMaxLine = (int64_t)1 << 30;      // a longer line cannot become a record (block_size is an int32)
constexpr uint32_t kMaxCigarLen = (1u << 28) - 1;
constexpr int64_t kMaxCigarOps = 65535;

// The reference names as the lookup reads them: name r = bytes[off[r], off[r + 1]), slot[] = an open-addressing table
// of mask + 1 entries (a power of two, at least twice the names, so an empty slot ends every probe), -1 = empty.
struct Names {
  const uint8_t* bytes;
  const int32_t* off;
  const int32_t* slot;
  uint32_t mask;
  int32_t nref;
};
// The hash of a name, order-independent over its bytes so that the lanes of an Io can add their shares.
UC_HD inline uint64_t name_term(uint64_t i, uint8_t b) {
  return bam::mix64((i + 1) * 0x9e3779b97f4a7c15ull + ((uint64_t)b + 1) * 0xd6e8feb86659fd93ull);
}
UC_HD inline uint64_t name_finish(uint64_t sum, uint64_t len) { return bam::mix64(sum ^ (len * 0xa0761d6478bd642full)); }

// What measure leaves for encode: f[k] = the start of mandatory field k (0..10) relative to the line, f[11] = one past
// the tab (or the line end) that closes field 10 = the start of the aux fields; field k is [f[k], f[k + 1] - 1).
struct Fields {
  int32_t f[12];
};
struct Measured {
  int32_t status = 0;  // code | field << 8
  int32_t nf = 0;      // aux fields of type f
  int64_t size = 0;    // bytes of the record, its block_size field included
  uint64_t key = 0;    // the sort key
};
// one aux f value the host has to fill: four bytes at raw[at], from the text at body[text ...] of input line `line`
struct FSlot {
  int64_t at, text, line;
};

// tid (-1 last) << 32 | (pos + 1) << 1 | reverse: samtools' bam1_cmp_core for SO:coordinate.  pos + 1 is the POS
// field, 0 .. 2^31 - 1, and the tid of a record without one is nref: 63 bits at the most.
UC_HD inline uint64_t sort_key(int32_t tid, int32_t pos, uint32_t flag, int32_t nref) {
  return ((uint64_t)(uint32_t)(tid < 0 ? nref : tid) << 32) | ((uint64_t)(uint32_t)(pos + 1) << 1) |
         ((flag & bam::kFlagReverse) ? 1u : 0u);
}
// the 4-bit code of a base, the inverse of bam::seq_symbol: case-insensitive, anything else 15
UC_HD inline uint32_t seq_code(uint8_t c) {
  switch (c >= 'a' && c <= 'z' ? c - 32 : c) {
    case '=': return 0;
    case 'A': return 1;
    case 'C': return 2;
    case 'M': return 3;
    case 'G': return 4;
    case 'R': return 5;
    case 'S': return 6;
    case 'V': return 7;
    case 'T': return 8;
    case 'W': return 9;
    case 'Y': return 10;
    case 'H': return 11;
    case 'K': return 12;
    case 'D': return 13;
    case 'B': return 14;
    default: return 15;
  }
}
// the op code of a CIGAR letter in "MIDNSHP=X", -1 for any other byte
UC_HD inline int32_t cigar_op(uint8_t c) {
  switch (c) {
    case 'M': return 0;
    case 'I': return 1;
    case 'D': return 2;
    case 'N': return 3;
    case 'S': return 4;
    case 'H': return 5;
    case 'P': return 6;
    case '=': return 7;
    case 'X': return 8;
    default: return -1;
  }
}

// 1..10 decimal digits at [s, t); the same on every lane (each reads the same bytes)
template <class Io>
UC_HD inline bool parse_u(Io& io, int64_t s, int64_t t, uint64_t& v) {
  v = 0;
  if (t <= s || t - s > 10) return false;
  for (int64_t p = s; p < t; p++) {
    const uint32_t d = (uint32_t)io.at(p) - '0';
    if (d > 9) return false;
    v = v * 10 + d;
  }
  return true;
}
// the same with an optional '-' in front: the magnitude and the sign
template <class Io>
UC_HD inline bool parse_i(Io& io, int64_t s, int64_t t, uint64_t& mag, bool& neg) {
  neg = t > s && io.at(s) == '-';
  return parse_u(io, s + (neg ? 1 : 0), t, mag);
}

// The reference whose name is the text at [s, t), or -2.  The lanes share the hash and the comparison.
template <class Io>
UC_HD inline int32_t lookup(Io& io, const Names& N, int64_t s, int64_t t) {
  const int64_t len = t - s;
  uint64_t part = 0;
  for (int64_t i = io.lane(); i < len; i += io.lanes()) part += name_term((uint64_t)i, io.at(s + i));
  const uint64_t h = name_finish(io.sum(part), (uint64_t)len);
  for (uint32_t k = (uint32_t)h & N.mask;; k = (k + 1) & N.mask) {
    const int32_t r = N.slot[k];
    if (r < 0) return -2;
    if ((int64_t)(N.off[r + 1] - N.off[r]) != len) continue;
    bool differs = false;
    for (int64_t i = io.lane(); i < len; i += io.lanes()) differs |= N.bytes[N.off[r] + i] != io.at(s + i);
    if (!io.any(differs)) return r;
  }
}

// the length in front of the op letter at p (p > s: digits run back from p - 1, at most 9 of them); 0 = refused
template <class Io>
UC_HD inline uint32_t cigar_len_before(Io& io, int64_t s, int64_t p) {
  uint32_t v = 0, mul = 1;
  int nd = 0;
  for (int64_t q = p; q > s && nd < 10; q--, nd++) {
    const uint32_t d = (uint32_t)io.at(q - 1) - '0';
    if (d > 9) break;
    if (nd < 9) v += d * mul, mul *= 10;
  }
  return nd == 0 || nd > 9 || v > kMaxCigarLen ? 0u : v;
}

// The mandatory fields of one line, parsed and checked.
struct Fixed {
  int32_t tid, pos, mapq, flag, ntid, npos, tlen, lname, lseq, ncig;
  int64_t rlen;       // M/D/N/=/X sum
  bool qual_missing;
};
template <class Io>
UC_HD inline int32_t parse_fixed(Io& io, const Names& N, int64_t b, const Fields& F, Fixed& X) {
  const auto fs = [&](int k) { return b + F.f[k]; };
  const auto fe = [&](int k) { return b + F.f[k + 1] - 1; };
  for (int k = 0; k < 11; k++)
    if (fe(k) <= fs(k)) return bad(kEFormat, k + 1);
  uint64_t v = 0;
  bool neg = false;
  // QNAME: 1..254 bytes
  if (fe(0) - fs(0) > 254) return bad(kEFormat, kFQname);
  X.lname = (int32_t)(fe(0) - fs(0)) + 1;
  if (!parse_u(io, fs(1), fe(1), v) || v > 65535) return bad(kEFormat, kFFlag);
  X.flag = (int32_t)v;
  const auto name = [&](int k, int32_t same, int32_t& out) {
    if (fe(k) - fs(k) == 1 && io.at(fs(k)) == '*') return out = -1, true;
    if (same != -3 && fe(k) - fs(k) == 1 && io.at(fs(k)) == '=') return out = same, true;
    out = lookup(io, N, fs(k), fe(k));
    return out >= 0;
  };
  if (!name(2, -3, X.tid)) return bad(kEFormat, kFRname);
  if (!parse_u(io, fs(3), fe(3), v) || v > 0x7fffffffu) return bad(kEFormat, kFPos);
  X.pos = (int32_t)v - 1;
  if (!parse_u(io, fs(4), fe(4), v) || v > 255) return bad(kEFormat, kFMapq);
  X.mapq = (int32_t)v;
  // CIGAR: every byte is a digit or an op letter with 1..9 digits in front of it, and the last one is a letter
  X.ncig = 0, X.rlen = 0;
  if (!(fe(5) - fs(5) == 1 && io.at(fs(5)) == '*')) {
    const int64_t s = fs(5), t = fe(5);
    uint64_t nops = 0, rl = 0;
    bool wrong = false;
    for (int64_t p = s + io.lane(); p < t; p += io.lanes()) {
      const uint8_t c = io.at(p);
      if (c >= '0' && c <= '9') {
        wrong |= p == t - 1;
        continue;
      }
      const int32_t op = cigar_op(c);
      const uint32_t ln = op < 0 ? 0u : cigar_len_before(io, s, p);
      wrong |= ln == 0;
      nops++;
      if (bam::op_on_reference((uint32_t)op)) rl += ln;
    }
    if (io.any(wrong)) return bad(kEFormat, kFCigar);
    nops = io.sum(nops), rl = io.sum(rl);
    if ((int64_t)nops > kMaxCigarOps) return bad(kERange, kFCigar);
    X.ncig = (int32_t)nops, X.rlen = (int64_t)rl;
  }
  if (!name(6, X.tid, X.ntid)) return bad(kEFormat, kFRnext);
  if (!parse_u(io, fs(7), fe(7), v) || v > 0x7fffffffu) return bad(kEFormat, kFPnext);
  X.npos = (int32_t)v - 1;
  if (!parse_i(io, fs(8), fe(8), v, neg) || v > (neg ? 0x80000000ull : 0x7fffffffull)) return bad(kEFormat, kFTlen);
  X.tlen = neg ? (int32_t)(0 - (uint32_t)v) : (int32_t)v;
  X.lseq = fe(9) - fs(9) == 1 && io.at(fs(9)) == '*' ? 0 : (int32_t)(fe(9) - fs(9));
  X.qual_missing = fe(10) - fs(10) == 1 && io.at(fs(10)) == '*';
  if (!X.qual_missing && fe(10) - fs(10) != X.lseq) return bad(kEFormat, kFQual);
  return kOk;
}

// The aux fields at [a, e) (one or more, tab-separated), sized, and with kWrite put at record offset o on.  o ends
// as the offset past the last one; nf counts the f values, each of which is left as four zero bytes and reported
// through io.fslot(record offset, text position).
template <bool kWrite, class Io>
UC_HD inline int32_t aux_walk(Io& io, int64_t a, int64_t e, int64_t& o, int32_t& nf) {
  for (int64_t s = a, t;; s = t + 1) {
    t = io.find(s, e, '\t');
    if (t - s < 5 || io.at(s + 2) != ':' || io.at(s + 4) != ':') return bad(kEFormat, kFAux);
    const uint8_t ty = io.at(s + 3);
    const int64_t v = s + 5;
    if (kWrite && io.lane() == 0) io.put(o, io.at(s)), io.put(o + 1, io.at(s + 1));
    if (ty == 'A') {
      if (t - v != 1) return bad(kEFormat, kFAux);
      if (kWrite && io.lane() == 0) io.put(o + 2, 'A'), io.put(o + 3, io.at(v));
      o += 4;
    } else if (ty == 'i') {
      // the smallest type that holds the value, as htslib chooses it
      uint64_t m = 0;
      bool neg = false;
      if (!parse_i(io, v, t, m, neg) || m > (neg ? 0x80000000ull : 0xffffffffull)) return bad(kEFormat, kFAux);
      if (m == 0) neg = false;
      const uint8_t code = neg ? (m <= 128 ? 'c' : m <= 32768 ? 's' : 'i') : (m <= 255 ? 'C' : m <= 65535 ? 'S' : 'I');
      const int w = bam::aux_fixed_size(code);
      if (kWrite && io.lane() == 0) {
        const uint32_t bits = neg ? 0u - (uint32_t)m : (uint32_t)m;
        io.put(o + 2, code);
        for (int k = 0; k < w; k++) io.put(o + 3 + k, (uint8_t)(bits >> (8 * k)));
      }
      o += 3 + w;
    } else if (ty == 'f') {
      if (t == v) return bad(kEFormat, kFAux);
      if (kWrite && io.lane() == 0) {
        io.put(o + 2, 'f');
        for (int k = 0; k < 4; k++) io.put(o + 3 + k, 0);
        io.fslot(o + 3, v);
      }
      nf++;
      o += 7;
    } else if (ty == 'Z' || ty == 'H') {
      if (kWrite) {
        if (io.lane() == 0) io.put(o + 2, ty), io.put(o + 3 + (t - v), 0);
        for (int64_t i = io.lane(); i < t - v; i += io.lanes()) io.put(o + 3 + i, io.at(v + i));
      }
      o += 3 + (t - v) + 1;
    } else {
      return bad(kEFormat, kFAux);
    }
    if (t >= e) return kOk;
  }
}

// The line body[b, e): its field table into F, its size, key and status.  nref = N.nref.
template <class Io>
UC_HD inline Measured measure(Io& io, const Names& N, int64_t b, int64_t e, Fields& F) {
  Measured M;
  for (int k = 0; k < 12; k++) F.f[k] = 0;
  if (e <= b) return M.status = bad(kEFormat, kFLine), M;
  if (e - b > kMaxLine) return M.status = bad(kERange, kFLine), M;
  int64_t s = b;
  for (int k = 0; k < 11; k++) {
    if (s > e) return M.status = bad(kEFormat, kFLine), M;  // fewer than 11 fields
    F.f[k] = (int32_t)(s - b);
    s = io.find(s, e, '\t') + 1;
  }
  F.f[11] = (int32_t)(s - b);
  Fixed X;
  if ((M.status = parse_fixed(io, N, b, F, X)) != kOk) return M;
  int64_t o = bam::aux_offset(X.lname, X.ncig, X.lseq);
  if (s <= e && (M.status = aux_walk<false>(io, s, e, o, M.nf)) != kOk) return M;
  if (o > 0x7fffffff) return M.status = bad(kERange, kFLine), M;
  M.size = o;
  M.key = sort_key(X.tid, X.pos, (uint32_t)X.flag, N.nref);
  return M;
}

// The record of the measured line body[b, e) through io.put(offset in the record, byte).
template <class Io>
UC_HD inline void encode(Io& io, const Names& N, int64_t b, int64_t e, const Fields& F, int64_t size) {
  Fixed X;
  if (parse_fixed(io, N, b, F, X) != kOk) return;  // (measure accepted the line)
  const auto fs = [&](int k) { return b + F.f[k]; };
  if (io.lane() == 0) {
    const auto put32 = [&](int64_t o, uint32_t v) {
      for (int k = 0; k < 4; k++) io.put(o + k, (uint8_t)(v >> (8 * k)));
    };
    const auto put16 = [&](int64_t o, uint32_t v) { io.put(o, (uint8_t)v), io.put(o + 1, (uint8_t)(v >> 8)); };
    // bin: the reference span of a mapped record with a CIGAR, else 1
    const int64_t rlen = bam::reference_span(!(X.flag & bam::kFlagUnmapped) && X.ncig ? X.rlen : 1);
    put32(bam::kBlockSize, (uint32_t)(size - 4));
    put32(bam::kRefId, (uint32_t)X.tid), put32(bam::kPos, (uint32_t)X.pos);
    io.put(bam::kLReadName, (uint8_t)X.lname), io.put(bam::kMapq, (uint8_t)X.mapq);
    put16(bam::kBin, (uint32_t)bam::reg2bin(X.pos, (int64_t)X.pos + rlen));
    put16(bam::kNCigarOp, (uint32_t)X.ncig), put16(bam::kFlag, (uint32_t)X.flag);
    put32(bam::kLSeq, (uint32_t)X.lseq), put32(bam::kNextRefId, (uint32_t)X.ntid);
    put32(bam::kNextPos, (uint32_t)X.npos), put32(bam::kTlen, (uint32_t)X.tlen);
    io.put(bam::kName + X.lname - 1, 0);
  }
  int64_t o = bam::kName;
  for (int64_t i = io.lane(); i < X.lname - 1; i += io.lanes()) io.put(o + i, io.at(fs(0) + i));
  o += X.lname;
  // CIGAR: op k of the text is word k; a step of lanes() bytes ranks its letters among themselves
  if (X.ncig) {
    const int64_t s = fs(5), t = b + F.f[6] - 1;
    int64_t k = 0;
    for (int64_t q = s; q < t; q += io.lanes()) {
      const int64_t p = q + io.lane();
      const int32_t op = p < t ? cigar_op(io.at(p)) : -1;
      int total = 0;
      const int r = io.rank(op >= 0, total);
      if (op >= 0) {
        const uint32_t w = (cigar_len_before(io, s, p) << 4) | (uint32_t)op;
        for (int x = 0; x < 4; x++) io.put(o + 4 * (k + r) + x, (uint8_t)(w >> (8 * x)));
      }
      k += total;
    }
    o += 4 * (int64_t)X.ncig;
  }
  // SEQ: two bases a byte, the first in the high half; QUAL: minus 33, or 0xff for '*'
  const int64_t half = (X.lseq + 1) / 2;
  for (int64_t j = io.lane(); j < half; j += io.lanes()) {
    const uint32_t hi = seq_code(io.at(fs(9) + 2 * j));
    const uint32_t lo = 2 * j + 1 < X.lseq ? seq_code(io.at(fs(9) + 2 * j + 1)) : 0u;
    io.put(o + j, (uint8_t)((hi << 4) | lo));
  }
  o += half;
  for (int64_t i = io.lane(); i < X.lseq; i += io.lanes())
    io.put(o + i, X.qual_missing ? 0xff : (uint8_t)(io.at(fs(10) + i) - 33));
  o += X.lseq;
  int32_t nf = 0;
  if (b + F.f[11] <= e) (void)aux_walk<true>(io, b + F.f[11], e, o, nf);
}

// ---------------------------------------------------------------- the host's part: header, name table, restatement
// The leading '@' lines of a SAM text, as the BAM holds them.
struct Header {
  std::vector<uint8_t> bam;  // "BAM\1", l_text, the text, n_ref, the references: what raw begins with
  std::vector<std::string> ref_name;
  std::vector<int64_t> ref_len;
  size_t body = 0;    // offset of the first record line in the text
  int64_t lines = 0;  // header lines, for the 1-based line numbers of the refusals
};
// The text is the header lines verbatim but for @HD: SO: becomes coordinate (added where it is missing), GO: goes,
// and a header without @HD gets "@HD\tVN:1.6\tSO:coordinate\n" in front.  No @PG line is added.  References from @SQ
// SN: / LN: in order; a duplicate SN, a missing field or an LN outside 1 .. 2^31 - 1 is refused.
inline bool build_header(const uint8_t* t, size_t n, Header& H, std::string& err) {
  std::string text;
  std::unordered_set<std::string> seen;
  bool have_hd = false;
  size_t o = 0;
  const auto refuse = [&](const char* what) {
    err = "line " + std::to_string(H.lines) + ": " + what;
    return false;
  };
  while (o < n && t[o] == '@') {
    const uint8_t* nl = (const uint8_t*)memchr(t + o, '\n', n - o);
    const size_t end = nl ? (size_t)(nl - t) : n;
    const std::string line((const char*)t + o, end - o);
    H.lines++;
    std::vector<std::string> fld;
    for (size_t s = 0;;) {
      const size_t tab = line.find('\t', s);
      fld.push_back(line.substr(s, tab == std::string::npos ? tab : tab - s));
      if (tab == std::string::npos) break;
      s = tab + 1;
    }
    if (fld[0] == "@HD" && !have_hd) {
      have_hd = true;
      std::string out = "@HD";
      bool so = false;
      for (size_t k = 1; k < fld.size(); k++) {
        if (fld[k].compare(0, 3, "GO:") == 0) continue;
        if (fld[k].compare(0, 3, "SO:") == 0) so = true;
        out += "\t" + (fld[k].compare(0, 3, "SO:") == 0 ? std::string("SO:coordinate") : fld[k]);
      }
      if (!so) out += "\tSO:coordinate";
      text += out + "\n";
    } else {
      text += line + "\n";
    }
    if (fld[0] == "@SQ") {
      std::string sn;
      int64_t ln = -1;
      bool has_sn = false;
      for (size_t k = 1; k < fld.size(); k++) {
        if (fld[k].compare(0, 3, "SN:") == 0 && !has_sn) sn = fld[k].substr(3), has_sn = true;
        if (fld[k].compare(0, 3, "LN:") == 0 && ln < 0) {
          const std::string d = fld[k].substr(3);
          if (d.empty() || d.size() > 10 || d.find_first_not_of("0123456789") != std::string::npos)
            return refuse("@SQ LN is no number");
          ln = strtoll(d.c_str(), nullptr, 10);
          if (ln < 1 || ln > 0x7fffffffLL) return refuse("@SQ LN outside 1 .. 2^31 - 1");
        }
      }
      if (!has_sn || sn.empty() || ln < 0) return refuse("@SQ without SN or LN");
      if (!seen.insert(sn).second) return refuse("@SQ SN is a duplicate");
      H.ref_name.push_back(sn), H.ref_len.push_back(ln);
    }
    o = nl ? end + 1 : n;
  }
  H.body = o;
  if (!have_hd) text = "@HD\tVN:1.6\tSO:coordinate\n" + text;
  if (text.size() > 0x7fffffffu) return err = "header text over 2 GiB", false;
  const auto put32 = [&](uint32_t v) {
    for (int k = 0; k < 4; k++) H.bam.push_back((uint8_t)(v >> (8 * k)));
  };
  H.bam.assign({'B', 'A', 'M', 1});
  put32((uint32_t)text.size());
  H.bam.insert(H.bam.end(), text.begin(), text.end());
  put32((uint32_t)H.ref_name.size());
  for (size_t r = 0; r < H.ref_name.size(); r++) {
    put32((uint32_t)H.ref_name[r].size() + 1);
    H.bam.insert(H.bam.end(), H.ref_name[r].begin(), H.ref_name[r].end());
    H.bam.push_back(0);
    put32((uint32_t)H.ref_len[r]);
  }
  return true;
}

// the lookup table of Names, owned
struct NameTable {
  std::vector<uint8_t> bytes;
  std::vector<int32_t> off, slot;
  uint32_t mask = 1;
  void build(const std::vector<std::string>& names) {
    off.assign(1, 0);
    for (const std::string& s : names) {
      bytes.insert(bytes.end(), s.begin(), s.end());
      off.push_back((int32_t)bytes.size());
    }
    bytes.push_back(0);
    uint64_t m = 2;
    while (m < 2 * (uint64_t)names.size()) m <<= 1;
    mask = (uint32_t)(m - 1);
    slot.assign((size_t)m, -1);
    for (size_t r = 0; r < names.size(); r++) {
      uint64_t sum = 0;
      for (size_t i = 0; i < names[r].size(); i++) sum += name_term(i, (uint8_t)names[r][i]);
      uint32_t k = (uint32_t)name_finish(sum, names[r].size()) & mask;
      while (slot[k] >= 0) k = (k + 1) & mask;
      slot[k] = (int32_t)r;
    }
  }
  Names view() const { return {bytes.data(), off.data(), slot.data(), mask, (int32_t)off.size() - 1}; }
};

// The record lines of body[0, n): start[l] for every line and one entry more, so that line l is
// [start[l], start[l + 1] - 1).  A last line without '\n' is a line.
inline void split_lines(const uint8_t* body, size_t n, std::vector<int64_t>& start) {
  start.clear();
  if (!n) return;
  start.push_back(0);
  for (size_t p = 0; p + 1 < n; p++)
    if (body[p] == '\n') start.push_back((int64_t)p + 1);
  start.push_back((int64_t)n + (body[n - 1] != '\n'));
}

// the plain serial Io: one lane
struct HostIo {
  const uint8_t* body;
  uint8_t* rec = nullptr;             // the record being written
  int64_t rec_at = 0, line = 0;       // its offset in raw, its input line
  std::vector<FSlot>* slots = nullptr;
  int lane() const { return 0; }
  int lanes() const { return 1; }
  uint8_t at(int64_t p) const { return body[p]; }
  int64_t find(int64_t s, int64_t e, uint8_t c) const {
    const void* q = e > s ? memchr(body + s, c, (size_t)(e - s)) : nullptr;
    return q ? (const uint8_t*)q - body : e;
  }
  uint64_t sum(uint64_t v) const { return v; }
  bool any(bool v) const { return v; }
  int rank(bool v, int& total) const { return total = v, 0; }
  void put(int64_t o, uint8_t b) { rec[o] = b; }
  void fslot(int64_t o, int64_t text) { slots->push_back({rec_at + o, text, line}); }
};

// (float)strtod(text) of the value at body[p ...] up to its tab, line end or n, as four little-endian bytes; false
// when strtod does not take the whole value
inline bool float_bytes(const uint8_t* body, size_t n, int64_t p, uint8_t out[4]) {
  size_t q = (size_t)p;
  while (q < n && body[q] != '\t' && body[q] != '\n') q++;
  const std::string s((const char*)body + p, q - (size_t)p);
  char* end = nullptr;
  const float f = (float)strtod(s.c_str(), &end);
  if (s.empty() || end != s.c_str() + s.size()) return false;
  memcpy(out, &f, 4);
  return true;
}

// "line L: FIELD: what" for a refused line (1-based L counts the header lines); an unknown reference is named.
// *status (may be null) = the line's status
inline std::string describe(const uint8_t* body, int64_t b, int64_t e, const Names& N, int64_t line_no,
                            int32_t* status = nullptr) {
  HostIo io{body};
  Fields F;
  const Measured M = measure(io, N, b, e, F);
  if (status) *status = M.status;
  if (M.status == kOk) return "line " + std::to_string(line_no) + ": refused on the device, accepted on the host";
  const int32_t field = M.status >> 8, code = M.status & 0xff;
  std::string what = "line " + std::to_string(line_no) + ": " + field_name(field) + ": ";
  if (field == kFLine)
    return what + (e <= b ? "empty line" : code == kERange ? "record over 2 GiB" : "fewer than 11 fields");
  if (code == kERange) return what + "more than 65535 CIGAR operations";
  if (field == kFRname || field == kFRnext) {
    const int64_t s = b + F.f[field - 1], t = b + F.f[field] - 1;
    return what + "unknown reference name '" + std::string((const char*)body + s, (size_t)std::max<int64_t>(0, t - s)) + "'";
  }
  return what + "malformed";
}

// The whole conversion on the host, serially: what the kernels of samsort.hip compute.  raw = the inflated BAM,
// roff = its record offsets.  Returns kOk, kEFormat or kERange with err set; raw is empty then.
inline int32_t encode_host(const uint8_t* text, size_t n, std::vector<uint8_t>& raw, std::vector<int64_t>& roff,
                           std::string& err) {
  raw.clear(), roff.clear();
  Header H;
  if (!build_header(text, n, H, err)) return kEFormat;
  NameTable T;
  T.build(H.ref_name);
  const Names N = T.view();
  const uint8_t* body = text + H.body;
  const size_t bn = n - H.body;
  std::vector<int64_t> start;
  split_lines(body, bn, start);
  const size_t nl = start.empty() ? 0 : start.size() - 1;
  std::vector<Fields> F(nl);
  std::vector<Measured> M(nl);
  HostIo io{body};
  for (size_t l = 0; l < nl; l++) {
    M[l] = measure(io, N, start[l], start[l + 1] - 1, F[l]);
    if (M[l].status != kOk) {
      err = describe(body, start[l], start[l + 1] - 1, N, H.lines + (int64_t)l + 1);
      return M[l].status & 0xff;
    }
  }
  std::vector<size_t> order(nl);
  for (size_t l = 0; l < nl; l++) order[l] = l;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return M[a].key < M[b].key; });
  int64_t total = (int64_t)H.bam.size();
  for (size_t l : order) roff.push_back(total), total += M[l].size;
  raw.assign((size_t)total, 0);
  memcpy(raw.data(), H.bam.data(), H.bam.size());
  std::vector<FSlot> slots;
  io.slots = &slots;
  for (size_t r = 0; r < nl; r++) {
    const size_t l = order[r];
    io.rec = raw.data() + roff[r], io.rec_at = roff[r], io.line = (int64_t)l;
    encode(io, N, start[l], start[l + 1] - 1, F[l], M[l].size);
  }
  for (const FSlot& s : slots)
    if (!float_bytes(body, bn, s.text, raw.data() + s.at)) {
      err = "line " + std::to_string(H.lines + s.line + 1) + ": aux: an f value is no number";
      raw.clear(), roff.clear();
      return kEFormat;
    }
  return kOk;
}

}  // namespace sam
}  // namespace uc
