// dropin_sam.cpp -- SAM text to the session's raw on the device (samsort.hip on sam_text.h): what
// umiclust_sam_open reads in place of a BAM file.  The rules of the text are in sam_text.h, HIP-free; this file uploads
// the text, runs the passes and carries the few values the host parses.
#include <cstring>

#include "bam_dev.h"
#include "sam_text.h"

using namespace uc;

// The sibling of read_bam_on_device for SAM text: the text uploaded, its lines split, measured, sorted and encoded on
// the device into d_raw -- the BAM header the host built, then the records in coordinate order -- and `raw` copied back
// to the host.  Text and raw are both on the device until this returns.  info: lines (header included), records, text
// bytes uploaded, aux f values the host parsed; times: upload, lines + measure, sort, encode, copy back in seconds by
// HIP events.  Fails the context: UMICLUST_EIO for a path that cannot be read, UMICLUST_EFORMAT / UMICLUST_ERANGE for
// a refused header or line (named), UMICLUST_ENOMEM for a device allocation that fails.
void uc::read_sam_on_device(Ctx* c, const char* path, RawBuf& raw, DevBuf<uint8_t>& d_raw, int64_t info[4],
                            double times[5]) {
  InputBytes in;
  if (!in.read(path, false)) c->fail(UMICLUST_EIO, "cannot read SAM %s", path);
  sam::Header H;
  std::string herr;
  if (!sam::build_header(in.p, in.n, H, herr)) c->fail(UMICLUST_EFORMAT, "%s: %s", path, herr.c_str());
  sam::NameTable T;
  T.build(H.ref_name);
  const uint8_t* const body = in.p + H.body;
  const int64_t N = (int64_t)(in.n - H.body), hdr_len = (int64_t)H.bam.size();
  const auto dev = [&](hipError_t e) {
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      c->fail(UMICLUST_ENOMEM, "device allocation failed");
    }
    c->hip(e, "alloc");
  };
  Event e[6];
  const auto mark = [&](int k) { c->hip(hipEventRecord(e[k].get(c), c->st), "event"); };
  // upload: the text after the header and the name table
  DevBuf<uint8_t> d_text, d_nbytes;
  DevBuf<int32_t> d_noff, d_nslot;
  dev(d_text.ensure((size_t)N + 1)), dev(d_nbytes.ensure(T.bytes.size())), dev(d_noff.ensure(T.off.size()));
  dev(d_nslot.ensure(T.slot.size()));
  mark(0);
  c->h2d(d_text.p, body, (size_t)N), c->h2d(d_nbytes.p, T.bytes.data(), T.bytes.size());
  c->h2d(d_noff.p, T.off.data(), T.off.size() * 4), c->h2d(d_nslot.p, T.slot.data(), T.slot.size() * 4);
  const sam::Names names{d_nbytes.p, d_noff.p, d_nslot.p, T.mask, (int32_t)H.ref_name.size()};
  mark(1);
  // lines
  int64_t n = 0;
  DevBuf<int64_t> d_cnt, d_first, d_start, d_one;
  dev(d_one.ensure(1));
  if (N > 0) {
    const size_t nc = (size_t)sam_line_chunks(N);
    dev(d_cnt.ensure(nc)), dev(d_first.ensure(nc));
    c->hip(launch_sam_count_lines(d_text.p, N, d_cnt.p, d_first.p, d_one.p, c->st), "sam lines");
    c->d2h(&n, d_one.p, 8);
    c->hip(hipStreamSynchronize(c->st), "sync");
    n += 1;
    if (n > INT32_MAX) c->fail(UMICLUST_ERANGE, "%s: more than 2^31 - 1 lines", path);
    dev(d_start.ensure((size_t)n + 1));
    c->hip(launch_sam_scatter_lines(d_text.p, N, d_first.p, n, d_start.p, c->st), "sam lines");
  }
  // measure: per line the field table, size, key and status
  const int64_t nb = (n + 255) / 256;
  DevBuf<sam::Fields> d_fields;
  DevBuf<int64_t> d_size, d_roff, d_hist;
  DevBuf<uint64_t> d_key, d_key2, d_acc;
  DevBuf<uint32_t> d_idx, d_idx2;
  DevBuf<int32_t> d_status;
  dev(d_fields.ensure((size_t)n)), dev(d_size.ensure((size_t)n)), dev(d_roff.ensure((size_t)n));
  dev(d_hist.ensure((size_t)nb * 256)), dev(d_key.ensure((size_t)n)), dev(d_key2.ensure((size_t)n));
  dev(d_acc.ensure(4)), dev(d_idx.ensure((size_t)n)), dev(d_idx2.ensure((size_t)n)), dev(d_status.ensure((size_t)n));
  uint64_t acc[4] = {~0ull, 0, 0, 0};  // first refused line, OR of the keys, aux f values, slots appended by encode
  c->h2d(d_acc.p, acc, sizeof(acc));
  c->hip(launch_sam_measure(d_text.p, d_start.p, n, names, d_fields.p, d_size.p, d_key.p, d_status.p, d_acc.p, c->st),
         "sam measure");
  c->d2h(acc, d_acc.p, sizeof(acc));
  mark(2);
  c->hip(hipStreamSynchronize(c->st), "sync");
  if (acc[0] != ~0ull) {
    // the refusal's text comes from the host restatement of the same rules, on that line alone
    int64_t be[2] = {0, 0};
    c->d2h(be, d_start.p + acc[0], 16);
    c->hip(hipStreamSynchronize(c->st), "sync");
    int32_t status = 0;
    const std::string what = sam::describe(body, be[0], be[1] - 1, T.view(), H.lines + (int64_t)acc[0] + 1, &status);
    c->fail((status & 0xff) == sam::kERange ? UMICLUST_ERANGE : UMICLUST_EFORMAT, "%s: %s", path, what.c_str());
  }
  // sort: stable by key
  const uint32_t* d_order = d_idx.p;
  c->hip(launch_sam_sort(d_key.p, d_idx.p, d_key2.p, d_idx2.p, n, acc[1], d_hist.p, &d_order, c->st), "sam sort");
  mark(3);
  // encode: roff, the header bytes, the records, the f values
  int64_t total = hdr_len;
  c->hip(launch_sam_roff(d_size.p, d_order, n, hdr_len, d_roff.p, d_one.p, c->st), "sam roff");
  c->d2h(&total, d_one.p, 8);
  c->hip(hipStreamSynchronize(c->st), "sync");
  const int64_t nf = (int64_t)acc[2];
  DevBuf<sam::FSlot> d_slots;
  dev(d_raw.ensure((size_t)total + 1)), dev(d_slots.ensure((size_t)nf));
  c->h2d(d_raw.p, H.bam.data(), H.bam.size());
  c->hip(launch_sam_encode(d_text.p, d_start.p, d_order, d_roff.p, n, names, d_fields.p, d_size.p, d_raw.p, d_slots.p,
                           d_acc.p + 3, nf, c->st),
         "sam encode");
  DevBuf<int64_t> d_at;
  DevBuf<uint32_t> d_bits;
  std::vector<int64_t> at((size_t)nf);
  std::vector<uint32_t> bits((size_t)nf);
  if (nf) {
    std::vector<sam::FSlot> slots((size_t)nf);
    c->d2h(slots.data(), d_slots.p, (size_t)nf * sizeof(sam::FSlot)), c->d2h(acc, d_acc.p, sizeof(acc));
    c->hip(hipStreamSynchronize(c->st), "sync");
    if ((int64_t)acc[3] != nf) c->fail(UMICLUST_EDEVICE, "%s: the encode pass listed %lld f values, the measure pass %lld",
                                       path, (long long)acc[3], (long long)nf);
    for (int64_t k = 0; k < nf; k++) {
      uint8_t b[4];
      if (!sam::float_bytes(body, (size_t)N, slots[k].text, b))
        c->fail(UMICLUST_EFORMAT, "%s: line %lld: aux: an f value is no number", path,
                (long long)(H.lines + slots[k].line + 1));
      at[k] = slots[k].at;
      memcpy(&bits[k], b, 4);
    }
    dev(d_at.ensure((size_t)nf)), dev(d_bits.ensure((size_t)nf));
    c->h2d(d_at.p, at.data(), (size_t)nf * 8), c->h2d(d_bits.p, bits.data(), (size_t)nf * 4);
    c->hip(launch_sam_put_f(d_raw.p, d_at.p, d_bits.p, nf, c->st), "sam put f");
  }
  mark(4);
  c->d2h(alloc_touched(raw, (size_t)total), d_raw.p, (size_t)total);
  mark(5);
  c->hip(hipStreamSynchronize(c->st), "sync");
  info[0] = H.lines + n, info[1] = n, info[2] = N, info[3] = nf;
  for (int x = 0; x < 5; x++) times[x] = elapsed_s(c, e[x], e[x + 1]);
}
