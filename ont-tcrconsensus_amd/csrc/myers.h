// myers.h -- the device side of the UMI search, shared by extract.hip (ASCII reads and gathered windows, row f1) and
// bamextract.hip (windows decoded from a BAM record's 4-bit sequence, row f4+f1).
//
// Myers' bit-parallel edit distance with the pattern (<= 64 symbols) in one 64-bit word, as edlib runs it for
// `edlib.align(pattern, window, task="path", mode="HW", k=max_pattern_dist, additionalEqualities=IUPAC)`:
//   HW pass: free target start (top row 0, no carry-in), bottom-row score tracked along the window; the
//     edit distance is the minimum (reported if <= k) and locations[0]'s end is the first column with it;
//   start pass (edlib obtainLocations for mode HW): SHW of the reversed pattern against the reversed window
//     prefix [0, end] (top row j: carry-in +1); the LAST reversed column with the edit distance gives
//     start = end - column.
// Equality is a 256-entry match mask per pattern (ExtractPatterns, built on the host).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "umiclust_internal.h"

namespace uc {

__device__ __forceinline__ void myers_step(uint64_t Eq, uint64_t mask, uint64_t hb, uint64_t hin, uint64_t& Pv,
                                           uint64_t& Mv, int& score) {
  const uint64_t Xv = Eq | Mv;
  const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  uint64_t Ph = Mv | ~(Xh | Pv);
  uint64_t Mh = Pv & Xh;
  score += (Ph & hb) ? 1 : ((Mh & hb) ? -1 : 0);
  Ph = (Ph << 1) | hin;
  Mh <<= 1;
  Pv = (Mh | ~(Xv | Ph)) & mask;
  Mv = Ph & Xv & mask;
}

// Both passes over the window of wl bytes that sym(j) yields (j in [0, wl)) against pattern w of P:
// o[0..2] = edit distance (-1: none <= k), start, end within the window.
template <typename Sym>
__device__ __forceinline__ void myers_locate(Sym sym, int wl, const ExtractPatterns* __restrict__ P, int w, int32_t k,
                                             int32_t* o) {
  const int m = P->m[w];
  const uint64_t* peq = P->peq[w];
  const uint64_t* peqr = P->peqr[w];
  const uint64_t mask = m == 64 ? ~0ull : ((1ull << m) - 1ull), hb = 1ull << (m - 1);
  uint64_t Pv = mask, Mv = 0;
  int score = m, best = 1 << 30, end = -1;
  for (int j = 0; j < wl; j++) {
    myers_step(peq[(uint8_t)sym(j)], mask, hb, 0ull, Pv, Mv, score);
    if (score < best) {
      best = score;
      end = j;
    }
  }
  if (end < 0 || best > k) {
    o[0] = -1;
    o[1] = -1;
    o[2] = -1;
    return;
  }
  Pv = mask;
  Mv = 0;
  score = m;
  int last = -1;
  for (int q = 0; q <= end; q++) {
    myers_step(peqr[(uint8_t)sym(end - q)], mask, hb, 1ull, Pv, Mv, score);
    if (score == best) last = q;
  }
  o[0] = best;
  o[1] = end - last;
  o[2] = end;
}

}  // namespace uc
