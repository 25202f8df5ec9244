// tunables.cpp -- the one reader of the UMICLUST_* environment variables (see tunables.h).
#include "tunables.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

extern char** environ;
namespace uc {

// The switches read below.  The enum and the names come from this one list and get() is the only way from here to the
// environment, so a switch the reader takes is a switch warn_unknown_env knows.
#define UC_SWITCHES(X)                                                                                         \
  X(BAND) X(BGZF_BATCH) X(BGZF_WRITE) X(BLOCK) X(DEBUG) X(FQ_CHUNK) X(IO_THREADS) X(MIXLEN) X(O4)              \
  X(OVERLAP_TEST_COLLIDE) X(PAR_MIN) X(PF1) X(PFPROBE) X(PFPROF) X(PIN) X(REGROW) X(RESOLVE_DUMP)              \
  X(RESOLVE_THREADS) X(SPLIT) X(WALK_DUMP)
#define UC_ENUM(n) k##n,
#define UC_NAME(n) "UMICLUST_" #n,
enum Switch { UC_SWITCHES(UC_ENUM) };
static const char* const kKnown[] = {UC_SWITCHES(UC_NAME)  // and those the Python side reads (umiclust/, bench.py):
    "UMICLUST_DEVICE", "UMICLUST_CRIT_PRIO", "UMICLUST_PACK_READS", "UMICLUST_BENCH_THREADS", "UMICLUST_E2E_DIR"};
static const char* get(Switch s) { return getenv(kKnown[s]); }

Tunables read_tunables() {
  Tunables t;
  if (const char* e = get(kBAND)) t.band_pairs = std::max(0, atoi(e));
  if (const char* e = get(kMIXLEN)) t.mix_len = atoi(e) != 0 ? 1 : 0;
  if (const char* e = get(kPAR_MIN)) t.par_min = std::max(1, atoi(e));
  if (const char* e = get(kPF1)) t.pf1_lds = std::max(0, atoi(e));
  if (const char* e = get(kREGROW)) t.regrow = std::max(0, atoi(e));
  if (const char* e = get(kFQ_CHUNK)) t.fq_chunk = std::max<int64_t>(1024, std::min<int64_t>(atoll(e), 1ll << 31));
  if (const char* e = get(kBGZF_WRITE)) t.bgzf_device = strcmp(e, "host") != 0;
  if (const char* e = get(kBGZF_BATCH)) t.bgzf_batch = std::max(1, std::min(atoi(e), 65536));
  if (const char* e = getenv("LOCAL_WORLD_SIZE")) t.pin = atoi(e) <= 1;
  if (const char* e = get(kPIN)) {
    t.pin = atoi(e) != 0;
    t.pin_forced = atoi(e) == 1;
  }
  if (const char* e = get(kSPLIT)) t.split_env = atoi(e) != 0 ? 1 : 0;
  if (const char* e = get(kRESOLVE_THREADS)) t.resolve_threads = std::max(1, std::min(16, atoi(e)));
  if (const char* e = get(kBLOCK)) {
    t.block_size = std::max(1, std::min(kTile, atoi(e)));
    t.block_div = 0;
  }
  t.pf_prof = get(kPFPROF) != nullptr;
  t.pf_probe = get(kPFPROBE) != nullptr;
  t.debug = env_debug();
  t.walk_dump = get(kWALK_DUMP);
  t.resolve_dump = get(kRESOLVE_DUMP);
  return t;
}

int env_debug() { return !get(kDEBUG) ? 0 : strcmp(get(kDEBUG), "2") == 0 ? 2 : 1; }
int env_io_threads() { return get(kIO_THREADS) ? std::max(1, std::min(atoi(get(kIO_THREADS)), 16)) : 0; }
const char* env_o4() { return get(kO4); }
bool env_overlap_test_collide() { return get(kOVERLAP_TEST_COLLIDE) != nullptr; }

void warn_unknown_env() {
  static std::once_flag once;
  std::call_once(once, [] {
    for (char** e = environ; e && *e; e++) {
      if (strncmp(*e, "UMICLUST_", 9) != 0) continue;
      const size_t len = strcspn(*e, "=");
      bool ok = false;
      for (const char* k : kKnown) ok = ok || (strlen(k) == len && strncmp(k, *e, len) == 0);
      if (!ok) fprintf(stderr, "umiclust: warning: unknown environment variable %.*s ignored (retired or misspelled)\n",
                       (int)len, *e);
    }
  });
}

}  // namespace uc
