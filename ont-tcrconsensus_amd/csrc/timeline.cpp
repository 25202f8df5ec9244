// timeline.cpp -- the process-wide timeline of the counting launches (kind 0) and the alignment chains (kind 1), for
// umiclust_timeline: with several contexts (lanes) on one device their HIP-event brackets overlap, so the sum of
// the brackets overstates the time the kernel held the device; the union of the intervals (interval_union.h), each
// taken against one reference event, does not.
#include <mutex>

#include "cluster_ctx.h"
#include "interval_union.h"

namespace uc {

namespace {

constexpr size_t kTlCap = 1 << 16, kTlKeep = 4096;  // keep the latest kTlKeep merged intervals unfolded (late arrivals)

struct Timeline {
  std::mutex m;
  hipEvent_t ref = nullptr;  // process lifetime: re-created only when the timeline moves to another device
  int dev = -1;
  IntervalUnion iv[2] = {{kTlCap, kTlKeep}, {kTlCap, kTlKeep}};  // ms since ref
  int64_t n[2] = {0, 0};
};
Timeline g_tl;

}  // namespace

void tl_add(int dev, int kind, hipEvent_t a, hipEvent_t b) {
  std::lock_guard<std::mutex> lk(g_tl.m);
  if (!g_tl.ref || dev != g_tl.dev) return;  // events of another device than the reference's: not comparable
  float t0 = 0.f, t1 = 0.f;
  if (hipEventElapsedTime(&t0, g_tl.ref, a) != hipSuccess || hipEventElapsedTime(&t1, g_tl.ref, b) != hipSuccess) {
    (void)hipGetLastError();  // measurement only: never leave a sticky error for the caller's next launch check
    return;
  }
  g_tl.n[kind]++;
  g_tl.iv[kind].add(t0, t1);
}

}  // namespace uc

using namespace uc;

extern "C" int32_t umiclust_timeline(int32_t device_id, int32_t kind, int32_t reset, double* busy_s,
                                     int64_t* launches) {
  if (kind < 0 || kind > 1) return UMICLUST_EINVAL;
  std::lock_guard<std::mutex> lk(g_tl.m);
  if (reset) {
    int prev = -1;
    (void)hipGetDevice(&prev);  // the reset must not move the caller's thread to another device
    if (hipSetDevice(device_id) != hipSuccess) return UMICLUST_EDEVICE;
    if (g_tl.ref && g_tl.dev != device_id) {
      (void)hipEventDestroy(g_tl.ref);
      g_tl.ref = nullptr;
    }
    int32_t rc = 0;
    if (!g_tl.ref && hipEventCreate(&g_tl.ref) != hipSuccess) {
      g_tl.ref = nullptr;
      rc = UMICLUST_EDEVICE;
    }
    if (rc == 0 && (hipEventRecord(g_tl.ref, nullptr) != hipSuccess || hipEventSynchronize(g_tl.ref) != hipSuccess))
      rc = UMICLUST_EDEVICE;
    if (prev >= 0) (void)hipSetDevice(prev);
    if (rc) return rc;
    g_tl.dev = device_id;
    for (int k = 0; k < 2; k++) {
      g_tl.iv[k].clear();
      g_tl.n[k] = 0;
    }
  }
  if (busy_s) *busy_s = g_tl.iv[kind].measure() * 1e-3;
  if (launches) *launches = g_tl.n[kind];
  return 0;
}
