// bam_host.cpp -- see bam_host.h.  No HIP here: plain g++, also built with ASan + UBSan by the CPU suite.
#include "bam_host.h"

#include <fcntl.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <thread>

namespace uc {
namespace bam {

bool parse_header(const uint8_t* raw, size_t n, Header& h, std::string& err) {
  h = Header();
  if (n < 12 || memcmp(raw, "BAM\1", 4) != 0) {
    err = "not BAM";
    return false;
  }
  const int32_t lt = (int32_t)le32(raw + 4);
  if (lt < 0 || (size_t)lt > n - 12) {
    err = "truncated BAM header";
    return false;
  }
  h.text_len = (size_t)lt;
  size_t o = 8 + (size_t)lt;
  const int32_t nref = (int32_t)le32(raw + o);
  o += 4;
  if (nref < 0 || (size_t)nref > (n - o) / 8) {
    err = "truncated BAM header";
    return false;
  }
  h.ref_name.resize((size_t)nref);
  h.ref_len.resize((size_t)nref);
  for (int32_t r = 0; r < nref; r++) {
    if (n - o < 8) {
      err = "truncated BAM header";
      return false;
    }
    const int32_t ln = (int32_t)le32(raw + o);
    if (ln < 0 || (size_t)ln > n - o - 8) {
      err = "truncated BAM header";
      return false;
    }
    h.ref_name[r] = std::string((const char*)raw + o + 4, (size_t)std::max(0, ln - 1));
    h.ref_len[r] = (int64_t)(int32_t)le32(raw + o + 4 + (size_t)ln);
    o += 4 + (size_t)ln + 4;
  }
  h.end = o;
  return true;
}

bool record_offsets(const uint8_t* raw, size_t n, size_t start, std::vector<int64_t>& roff, std::string& err) {
  roff.clear();
  size_t o = start;
  while (o + 4 <= n) {
    const int32_t bs = (int32_t)le32(raw + o);
    if (bs < 32 || (size_t)bs > n - o - 4) {
      err = "truncated BAM record " + std::to_string(roff.size());
      return false;
    }
    roff.push_back((int64_t)o);
    o += 4 + (size_t)bs;
  }
  if (o != n) {
    err = "truncated BAM record " + std::to_string(roff.size());
    return false;
  }
  return true;
}

bool check_record_fields(const uint8_t* raw, const std::vector<int64_t>& roff, std::string& err) {
  for (size_t r = 0; r < roff.size(); r++) {
    const uint8_t* rec = raw + roff[r];
    const int64_t bs = block_size(rec), lrn = l_read_name(rec), ncig = n_cigar_op(rec), lseq = l_seq(rec);
    if (!fits(lrn, ncig, lseq, bs)) {
      err = "BAM record " + std::to_string(r) + ": l_read_name " + std::to_string(lrn) + ", n_cigar_op " +
            std::to_string(ncig) + ", l_seq " + std::to_string(lseq) + " do not fit block_size " + std::to_string(bs);
      return false;
    }
  }
  return true;
}

void scan_record(const uint8_t* raw, int64_t roff, uint64_t seed, uint64_t hmask, ScanRow& out) {
  out = ScanRow();
  const uint8_t* rec = raw + roff;
  const int64_t end = roff + 4 + (int64_t)block_size(rec);
  const uint32_t lrn = l_read_name(rec), ncig = n_cigar_op(rec), flag = bam::flag(rec);
  const int32_t lseq = l_seq(rec);
  out.ref = ref_id(rec);
  out.l_seq = lseq;
  out.cls = (flag & kFlagUnmapped) ? kScanUnmapped : (flag & kFlagNotPrimary) ? kScanSecondary : kScanPrimary;
  const int64_t aux = roff + aux_offset(lrn, ncig, lseq);
  if (lseq < 0 || aux > end) {
    out.bad = 1;
    return;
  }
  int64_t rl = 0, cols = 0;
  for (uint32_t x = 0; x < ncig; x++) {
    const uint32_t v = le32(cigar(rec, lrn) + 4 * (int64_t)x), op = v & 15u;
    if (op_on_reference(op)) rl += v >> 4;
    if (op_in_columns(op)) cols += v >> 4;
  }
  out.reference_length = reference_span(rl);
  out.cols = cols;
  if (out.cls != kScanPrimary) return;  // the reference never reads the tags of the other records
  bool have_nm = false, have_cs = false;
  int64_t cur = aux;
  while (cur < end) {
    if (cur + 3 > end) {
      out.bad = 1;
      return;
    }
    const uint8_t t0 = raw[cur], t1 = raw[cur + 1], ty = raw[cur + 2];
    const bool is_nm = t0 == 'N' && t1 == 'M' && !have_nm, is_cs = t0 == 'c' && t1 == 's' && !have_cs;
    const int64_t v = cur + 3;
    const int sz = aux_fixed_size(ty);
    if (sz) {
      if (v + sz > end || is_cs || (is_nm && (ty == 'A' || ty == 'f'))) {
        out.bad = 1;
        return;
      }
      if (is_nm) {
        out.nm = aux_int_value(ty, raw + v);
        out.nm_present = 1;
        have_nm = true;
      }
      cur = v + sz;
    } else if (ty == 'B') {
      if (v + 5 > end || is_nm || is_cs) {
        out.bad = 1;
        return;
      }
      const int64_t cnt = (int64_t)le32(raw + v + 1);
      const int ss = aux_array_elem_size(raw[v]);
      if (!ss || v + 5 + ss * cnt > end) {
        out.bad = 1;
        return;
      }
      cur = v + 5 + ss * cnt;
    } else if (ty == 'Z' || ty == 'H') {
      if (is_nm || (is_cs && ty != 'Z')) {
        out.bad = 1;
        return;
      }
      int64_t z = v;
      uint64_t sum = 0;
      while (z < end && raw[z] != 0) {
        if (is_cs) sum += cs_term(seed, (uint64_t)(z - v), raw[z]);
        z++;
      }
      if (z >= end) {  // no NUL before the record end
        out.bad = 1;
        return;
      }
      if (is_cs) {
        out.cs_off = v;
        out.cs_len = (int32_t)(z - v);
        out.cs_hash = cs_finish(sum, (uint64_t)(z - v), hmask);
        have_cs = true;
      }
      cur = z + 1;
    } else {
      out.bad = 1;
      return;
    }
  }
}

// ---------------------------------------------------------------- detected-UMI record (row f4+f1)
std::string forward_text(const uint8_t* rec) {
  const int32_t lseq = l_seq(rec);
  if (lseq <= 0) return "None";
  const uint8_t* sq = seq(rec, l_read_name(rec), n_cigar_op(rec));
  const bool rev = (flag(rec) & kFlagReverse) != 0;
  std::string out((size_t)lseq, '\0');
  for (int32_t x = 0; x < lseq; x++) out[(size_t)x] = forward_base(sq, lseq, rev, x);
  return out;
}

std::string format_umi_record(const uint8_t* rec, const int32_t* res, int32_t a3) {
  const std::string read = forward_text(rec);
  std::string hdr((const char*)name(rec), (size_t)l_read_name(rec) - 1);
  hdr += (flag(rec) & kFlagReverse) ? ";strand=-" : ";strand=+";
  const std::string rid = hdr.substr(0, hdr.find(';'));
  const size_t s0 = hdr.find("strand=") + 7, s1 = hdr.find("strand=", s0);
  const std::string strand = hdr.substr(s0, s1 == std::string::npos ? s1 : s1 - s0);
  const size_t L = read.size(), w3 = (a3 == 0 || (size_t)a3 > L) ? L : (size_t)a3;
  const std::string u5 = read.substr((size_t)res[1], (size_t)(res[2] - res[1] + 1));
  const std::string u3 = read.substr(L - w3 + (size_t)res[4], (size_t)(res[5] - res[4] + 1));
  std::string out = ">" + rid + ";strand=" + strand + ";umi_fwd_dist=" + std::to_string(res[0]) + ";umi_rev_dist=" +
                    std::to_string(res[3]) + ";umi_fwd_seq=" + u5 + ";umi_rev_seq=" + u3 + ";seq=" + read + "\n";
  if (strand == "+") {
    out += u5 + u3;
  } else {
    for (const std::string* u : {&u3, &u5})
      for (size_t x = u->size(); x-- > 0;) out.push_back(complement((*u)[x]));
  }
  out.push_back('\n');
  return out;
}

// ---------------------------------------------------------------- BGZF writer
const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                              0x02, 0,    0x1b, 0,    0x03, 0, 0, 0, 0, 0, 0, 0,    0,    0};

bool bgzf_block(const uint8_t* src, size_t n, std::vector<uint8_t>& out) {
  for (int level : {6, 0}) {
    out.assign(18 + compressBound((uLong)n) + 64 + 8, 0);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    zs.next_in = const_cast<Bytef*>(src);
    zs.avail_in = (uInt)n;
    zs.next_out = out.data() + 18;
    zs.avail_out = (uInt)(out.size() - 18 - 8);
    const int rc = deflate(&zs, Z_FINISH);
    const size_t clen = (size_t)zs.total_out;
    deflateEnd(&zs);
    if (rc != Z_STREAM_END) return false;
    const size_t total = 18 + clen + 8;
    if (total > 0x10000) continue;
    const uint8_t hdr[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};
    memcpy(out.data(), hdr, 16);
    out[16] = (uint8_t)((total - 1) & 0xff);
    out[17] = (uint8_t)((total - 1) >> 8);
    const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, (uInt)n);
    uint8_t* t = out.data() + 18 + clen;
    for (int x = 0; x < 4; x++) t[x] = (uint8_t)(crc >> (8 * x));
    for (int x = 0; x < 4; x++) t[4 + x] = (uint8_t)((uint32_t)n >> (8 * x));
    out.resize(total);
    return true;
  }
  return false;
}

bool write_fd(int fd, const uint8_t* p, size_t n) {
  while (n) {
    const ssize_t w = write(fd, p, n);
    if (w < 0) return false;
    p += w;
    n -= (size_t)w;
  }
  return true;
}

uint32_t bgzf_crc32(const uint8_t* p, size_t n) { return (uint32_t)crc32(crc32(0L, Z_NULL, 0), p, (uInt)n); }

BgzfStream bgzf_stream(const uint8_t* raw, size_t header_end, const std::vector<int64_t>& roff, const uint8_t* keep) {
  BgzfStream S;
  S.raw = raw;
  S.seg.emplace_back(0, header_end);
  for (size_t r = 0; r < roff.size(); r++)
    if (keep[r]) {
      const size_t o = (size_t)roff[r], n = 4 + (size_t)block_size(raw + o);
      if (S.seg.back().first + S.seg.back().second == o) S.seg.back().second += n;
      else S.seg.emplace_back(o, n);
      S.nkept++;
    }
  S.seg_at.assign(S.seg.size() + 1, 0);
  for (size_t k = 0; k < S.seg.size(); k++) S.seg_at[k + 1] = S.seg_at[k] + S.seg[k].second;
  S.total = S.seg_at.back();
  return S;
}

void BgzfStream::gather(size_t at, size_t n, uint8_t* dst) const {
  size_t k = (size_t)(std::upper_bound(seg_at.begin(), seg_at.end(), at) - seg_at.begin()) - 1, got = 0;
  for (size_t in_seg = at - seg_at[k]; got < n; k++, in_seg = 0) {
    const size_t m = std::min(n - got, seg[k].second - in_seg);
    memcpy(dst + got, raw + seg[k].first + in_seg, m);
    got += m;
  }
}

void bgzf_gather_crc(const BgzfStream& S, size_t b0, size_t b1, uint8_t* dst, uint32_t* crc, int threads) {
  const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), b1 - b0));
  std::atomic<size_t> next(b0);
  auto work = [&]() {
    for (size_t b = next.fetch_add(1); b < b1; b = next.fetch_add(1)) {
      const size_t n = S.block_bytes(b);
      uint8_t* const d = dst + (b - b0) * kBgzfPayload;
      S.gather(b * kBgzfPayload, n, d);
      crc[b - b0] = bgzf_crc32(d, n);
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
}

int64_t write_bgzf(const char* path, const uint8_t* raw, size_t header_end, const std::vector<int64_t>& roff,
                   const uint8_t* keep, int threads, std::string& err, std::vector<int64_t>* coff) {
  const BgzfStream S = bgzf_stream(raw, header_end, roff, keep);
  int64_t at = 0;
  if (coff) coff->clear();
  const size_t total = S.total;
  const int64_t nkept = S.nkept;
  const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
  if (fd < 0) {
    err = std::string("cannot create ") + path;
    return -1;
  }
  const size_t nb = (total + kBgzfPayload - 1) / kBgzfPayload;
  const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), nb));
  const size_t batch = (size_t)T * 16;  // blocks compressed before the next in-order write
  std::vector<std::vector<uint8_t>> out(std::min(batch, std::max<size_t>(nb, 1)));
  bool ok = true;
  for (size_t b0 = 0; b0 < nb && ok; b0 += batch) {
    const size_t b1 = std::min(nb, b0 + batch);
    std::atomic<size_t> next(b0);
    std::atomic<int> failed(0);
    auto work = [&]() {
      std::vector<uint8_t> in(kBgzfPayload);
      for (size_t b = next.fetch_add(1); b < b1; b = next.fetch_add(1)) {
        const size_t a = b * kBgzfPayload, n = std::min(kBgzfPayload, total - a);
        S.gather(a, n, in.data());  // the block's bytes
        if (!bgzf_block(in.data(), n, out[b - b0])) failed = 1;
      }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    ok = !failed;
    for (size_t b = b0; b < b1 && ok; b++) {
      ok = write_fd(fd, out[b - b0].data(), out[b - b0].size());
      if (coff) coff->push_back(at);
      at += (int64_t)out[b - b0].size();
    }
  }
  if (coff) coff->push_back(at);
  ok = ok && write_fd(fd, kBgzfEof, sizeof kBgzfEof);
  ok = (close(fd) == 0) && ok;
  if (!ok) {
    err = std::string("cannot write ") + path;
    return -1;
  }
  return nkept;
}

}  // namespace bam
}  // namespace uc
