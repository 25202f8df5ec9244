// bam_record.h -- the layout of one BAM record, stated once, HIP-free (SAM specification §4.2).
//
// Every reader of a record names these: the kernels of regionsplit.hip, bamsplit.hip, bamscan.hip, bamextract.hip and
// bamindex.hip, the rules of bam_index.h and sam_text.h, the host side in bam_host.cpp and the drop-ins.  A vocabulary,
// not a parser: no walk and no bounds policy lives here, each reader keeps its own (what it clamps, what it has had
// checked before it runs).  rec is always the record's block_size field, and every offset counts from there.
#pragma once
#include <stdint.h>

#ifndef UC_HD
#if defined(__HIPCC__)
#define UC_HD __host__ __device__
#else
#define UC_HD
#endif
#endif

namespace uc {
namespace bam {

// ---- little-endian loads, byte by byte: a record lies at any address
UC_HD inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
UC_HD inline uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// ---- the fixed part: offsets from the block_size field
enum : int {
  kBlockSize = 0, kRefId = 4, kPos = 8, kLReadName = 12, kMapq = 13, kBin = 14, kNCigarOp = 16, kFlag = 18, kLSeq = 20,
  kNextRefId = 24, kNextPos = 28, kTlen = 32, kName = 36
};
constexpr int kFixed = 36;  // block_size and the 32 fixed bytes it counts
// int32 block_size refID pos, uint8 l_read_name mapq, uint16 bin n_cigar_op flag, int32 l_seq next_refID next_pos tlen
static_assert(kRefId == kBlockSize + 4 && kPos == kRefId + 4 && kLReadName == kPos + 4 && kMapq == kLReadName + 1, "");
static_assert(kBin == kMapq + 1 && kNCigarOp == kBin + 2 && kFlag == kNCigarOp + 2 && kLSeq == kFlag + 2, "");
static_assert(kNextRefId == kLSeq + 4 && kNextPos == kNextRefId + 4 && kTlen == kNextPos + 4 && kName == kTlen + 4, "");
static_assert(kName == kFixed, "the name follows the fixed part");

UC_HD inline uint32_t block_size(const uint8_t* rec) { return le32(rec + kBlockSize); }  // the bytes after this field
UC_HD inline int32_t ref_id(const uint8_t* rec) { return (int32_t)le32(rec + kRefId); }
UC_HD inline int32_t pos(const uint8_t* rec) { return (int32_t)le32(rec + kPos); }
UC_HD inline uint32_t l_read_name(const uint8_t* rec) { return rec[kLReadName]; }  // with the NUL
UC_HD inline uint32_t mapq(const uint8_t* rec) { return rec[kMapq]; }
UC_HD inline uint32_t bin(const uint8_t* rec) { return le16(rec + kBin); }
UC_HD inline uint32_t n_cigar_op(const uint8_t* rec) { return le16(rec + kNCigarOp); }
UC_HD inline uint32_t flag(const uint8_t* rec) { return le16(rec + kFlag); }
UC_HD inline int32_t l_seq(const uint8_t* rec) { return (int32_t)le32(rec + kLSeq); }
UC_HD inline int32_t next_ref_id(const uint8_t* rec) { return (int32_t)le32(rec + kNextRefId); }
UC_HD inline int32_t next_pos(const uint8_t* rec) { return (int32_t)le32(rec + kNextPos); }
UC_HD inline int32_t tlen(const uint8_t* rec) { return (int32_t)le32(rec + kTlen); }

// ---- where the variable fields start: name, CIGAR words, 4-bit sequence, qualities, aux
UC_HD inline const uint8_t* name(const uint8_t* rec) { return rec + kName; }
UC_HD inline const uint8_t* cigar(const uint8_t* rec, uint32_t lrn) { return rec + kName + lrn; }
UC_HD inline const uint8_t* seq(const uint8_t* rec, uint32_t lrn, uint32_t n) { return rec + kName + lrn + 4 * n; }
// the offset of the aux fields = the size of a record without any (n CIGAR ops, l bases)
UC_HD inline int64_t aux_offset(int64_t lrn, int64_t n, int64_t l) { return kFixed + lrn + 4 * n + (l + 1) / 2 + l; }
// the variable fields stay inside the record
UC_HD inline bool fits(int64_t lrn, int64_t ncig, int64_t lseq, int64_t block_size) {
  return lrn >= 1 && lseq >= 0 && aux_offset(lrn, ncig, lseq) <= 4 + block_size;
}

// ---- flag bits
enum : uint32_t {
  kFlagUnmapped = 0x4, kFlagReverse = 0x10, kFlagSecondary = 0x100, kFlagQcFail = 0x200, kFlagSupplementary = 0x800,
  kFlagNotPrimary = kFlagSecondary | kFlagSupplementary
};

// ---- CIGAR: word = length << 4 | op, op in "MIDNSHP=X"
// M D N = X consume the reference; M I D are the columns of an alignment
UC_HD inline bool op_on_reference(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
UC_HD inline bool op_in_columns(uint32_t op) { return op <= 2; }
// htslib's bam_endpos: a zero reference span (no CIGAR, or only I/S/H/P ops) counts as 1
UC_HD inline int64_t reference_span(int64_t sum) { return sum ? sum : 1; }

// ---- the 4-bit sequence
// "=ACMGRSVTWYHKDBN"[code], the table in two registers
UC_HD inline char seq_symbol(uint32_t code) {
  const uint64_t lo = 0x565352474d43413dull, hi = 0x4e42444b48595754ull;
  return (char)(((code & 8u) ? hi : lo) >> ((code & 7u) * 8));
}
// A <-> T, C <-> G, every other byte unchanged
UC_HD inline char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }
// byte x of the forward read (pysam's get_forward_sequence): stored position x, or on the reverse strand stored
// position l_seq - 1 - x, complemented.  sq = seq(rec, ...), 0 <= x < lseq
UC_HD inline char forward_base(const uint8_t* sq, int32_t lseq, bool rev, int32_t x) {
  const int32_t y = rev ? lseq - 1 - x : x;
  const char ch = seq_symbol((sq[y >> 1] >> (((y & 1) ^ 1) * 4)) & 15u);
  return rev ? complement(ch) : ch;
}

// ---- the bin of [beg, end): htslib's hts_reg2bin(beg, end, 14, 5), on arithmetic shifts: beg = -1, end = 0 gives
// 4680.  The level offsets are ((1 << 15) - 1) / 7 = 4681, ((1 << 12) - 1) / 7 = 585, 73, 9 and 1, so for
// 0 <= beg < end <= 2^29 -- all the .bai index asks about -- this is the specification's int form, term by term.
UC_HD inline int32_t reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (int32_t)(4681 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (int32_t)(585 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (int32_t)(73 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (int32_t)(9 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (int32_t)(1 + (beg >> 26));
  return 0;
}

// ---- hashing
UC_HD inline uint64_t mix64(uint64_t h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}
// The hash of a cs string, order-independent over its bytes so that a wave can sum 64 positions a step:
// mix(sum over x of mix(seed + (x + 1) * K1 + (byte + 1) * K2) ^ len * K3) & hmask, kCsEmpty mapped to kCsEmpty - 1.
constexpr uint64_t kCsEmpty = ~0ull;  // the group table's empty key: never a cs_hash
constexpr uint64_t kCsK1 = 0x9e3779b97f4a7c15ull, kCsK2 = 0xd6e8feb86659fd93ull, kCsK3 = 0xa0761d6478bd642full;
UC_HD inline uint64_t cs_term(uint64_t seed, uint64_t x, uint8_t b) {
  return mix64(seed + (x + 1) * kCsK1 + ((uint64_t)b + 1) * kCsK2);
}
UC_HD inline uint64_t cs_finish(uint64_t sum, uint64_t len, uint64_t hmask) {
  const uint64_t h = mix64(sum ^ (len * kCsK3)) & hmask;
  return h == kCsEmpty ? h - 1 : h;
}
// seed of hashing pass k (pass 0 first; a detected collision moves on to k + 1)
UC_HD inline uint64_t cs_seed(int k) { return 0x243f6a8885a308d3ull + (uint64_t)k * 0x13198a2e03707345ull; }

// ---- aux leaves: tag[2] type value
// bytes of a fixed-size value (A c C s S i I f), 0 for any other type byte
UC_HD inline int aux_fixed_size(uint8_t type) {
  return (type == 'A' || type == 'c' || type == 'C') ? 1 : (type == 's' || type == 'S') ? 2
         : (type == 'i' || type == 'I' || type == 'f') ? 4 : 0;
}
// bytes of one element of a B array: the same types but A, 0 for any other subtype byte
UC_HD inline int aux_array_elem_size(uint8_t subtype) { return subtype == 'A' ? 0 : aux_fixed_size(subtype); }
// the value of an integer type (c C s S i I) at p
UC_HD inline int64_t aux_int_value(uint8_t type, const uint8_t* p) {
  return type == 'c' ? (int64_t)(int8_t)p[0] : type == 'C' ? (int64_t)p[0] : type == 's' ? (int64_t)(int16_t)le16(p)
         : type == 'S' ? (int64_t)le16(p) : type == 'i' ? (int64_t)(int32_t)le32(p) : (int64_t)le32(p);
}

}  // namespace bam
}  // namespace uc
