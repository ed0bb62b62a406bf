// Tuning switches: every OZK_* environment variable the native library reads is declared HERE and nowhere else.
// Plain C++ (no HIP header), so that tests/native/knobs_hostcheck.cpp compiles it with g++.
//
// Values are PROCESS-WIDE per generation: an immutable snapshot of the whole table is built at first use and at each
// env_reload(), under a mutex, and published through one atomic pointer.  A read is one acquire load and an array
// index: no lock, no strcmp.  Every thread therefore sees the same values until the next reload, whatever the
// environment did in between — an MSM's buffers sized on one thread and used by a stage on another are laid out for
// the same plan.  env_reload() (ozk_tuning_reload) is for tests and tuning scripts only: it must not run beside a
// call in flight, and the snapshots it replaces are kept until the process exits (a reader may still hold one).
// Parsing: unset or empty means the default, anything else is atoi().
#pragma once
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>

namespace ozk {

constexpr int KNOB_COMPUTED = -0x7fffffff;      // the default is computed by the caller: read with knob_or(K, computed)
constexpr int KNOB_STRING = KNOB_COMPUTED + 1;  // a string, read with knob_str(K) (nullptr when unset or empty)

//   identifier, environment name, default, meaning
#define OZK_KNOBS(X)                                                                                                     \
  /* variable-base MSM plan (msm_var_driver.cuh: make_plan, plan_for) */                                                 \
  X(MSM_GLV, "OZK_MSM_GLV", 1, "0: plain 256-bit windows instead of the GLV split (var MSM up to 2^23 pairs, fixed base)") \
  X(MSM_SIGNED, "OZK_MSM_SIGNED", 1, "0: unsigned window digits in the GLV form")                                        \
  X(MSM_C, "OZK_MSM_C", KNOB_COMPUTED, "window bits, 1..16 (default: the cost model's choice)")                          \
  X(MSM_L1, "OZK_MSM_L1", KNOB_COMPUTED, "sorted entries per level-1 lane (default: from the bucket size; 0 as unset)")   \
  X(MSM_L1_WHOLE, "OZK_MSM_L1_WHOLE", 1, "G1 level 1 by whole buckets on lane groups: 0 never, 1 on every plan that can take it (unset: where it pays)") \
  X(MSM_L1_ORDER, "OZK_MSM_L1_ORDER", 1, "item order of the whole-bucket level 1: 0 by rank inside the sort bin, 1 by part length over the whole MSM") \
  X(MSM_L1_DENSE, "OZK_MSM_L1_DENSE", 1, "0: every workgroup of the whole-bucket level 1 merges lane groups by quad permutes, none densely through LDS") \
  X(MSM_L1_ROUNDS, "OZK_MSM_L1_ROUNDS", 2, "most rounds of resident workgroups level 1 is rounded up to; 0: no rounding") \
  X(MSM_TAIL_MODE, "OZK_MSM_TAIL_MODE", -1, "0 / 1: force the latency / throughput shape of the window sums")            \
  X(MSM_TAIL_RC, "OZK_MSM_TAIL_RC", -1, "1: G1 throughput window sums by bucket rows and columns wherever the buffers take them (0 / unset: the serial levels)") \
  X(MSM_SMALL_SORT, "OZK_MSM_SMALL_SORT", 1, "0: small MSMs take the two-level sort too")                                \
  X(MSM_S_LAT, "OZK_MSM_S_LAT", KNOB_COMPUTED, "buckets per lane in a latency tail's fused first level (default: 8 G1, 4 G2)") \
  X(MSM_FIN_MAX, "OZK_MSM_FIN_MAX", 4, "elements per window left to the final one-wave kernel, 1..16")                   \
  /* host-buffer MSM */                                                                                                  \
  X(HOST_SLICES, "OZK_HOST_SLICES", 8, "most slices a host-buffer MSM is cut into; 1: no slicing")                       \
  X(HOST_SLICE_MIN_LOG, "OZK_HOST_SLICE_MIN_LOG", 18, "log2 of the smallest slice")                                      \
  X(SHARD, "OZK_SHARD", 0, "1: the JNI entries shard large calls over the visible devices")                              \
  X(SHARD_MIN_N, "OZK_SHARD_MIN_N", 1 << 21, "smallest call OZK_SHARD=1 shards")                                         \
  X(SHARD_COUNT, "OZK_SHARD_COUNT", 0, "shards of such a call; 0: one per device")                                       \
  X(SHARD_RCCL, "OZK_SHARD_RCCL", 1, "0: the partials of a sharded call go through the host, not RCCL")                  \
  X(COPY_HELPERS, "OZK_COPY_HELPERS", 3, "threads staging host buffers beside the caller, 0..11 (first use only)")       \
  X(HOST_TRACE, "OZK_HOST_TRACE", 0, "1: per-call host timings on stderr; 2: with absolute timestamps")                  \
  /* fixed-base and shared-base MSM */                                                                                   \
  X(FB_WS, "OZK_FB_WS", KNOB_COMPUTED, "window bits of a GLV fixed-base table (default: cost model, at most the caller's)") \
  X(FB_AFFINE, "OZK_FB_AFFINE", 1, "0: Jacobian gather-add instead of affine table records")                             \
  X(FB_TABLE_CACHE, "OZK_FB_TABLE_CACHE", 1, "0: window tables are built per call")                                      \
  X(FB_TABLE_CACHE_MB, "OZK_FB_TABLE_CACHE_MB", 1024, "MiB of cached window tables per device")                          \
  X(FB_TABLE_CACHE_SECOND_USE, "OZK_FB_TABLE_CACHE_SECOND_USE", 1, "0: a table is cached on its first use")              \
  X(FB_HOST_RANGES, "OZK_FB_HOST_RANGES", 4, "ranges a host fixed-base call downloads its results in")                   \
  X(MM_WS, "OZK_MM_WS", KNOB_COMPUTED, "window bits of the shared-base batched MSM (default: from n)")                   \
  /* FFT, witness map, BACE */                                                                                           \
  X(FFT_MAXK, "OZK_FFT_MAXK", 8, "most butterfly stages per pass, 3..10")                                                \
  X(FFT_PLAN, "OZK_FFT_PLAN", 1, "0: stages spread evenly over the passes")                                              \
  X(FFT_KS, "OZK_FFT_KS", KNOB_STRING, "explicit stages per pass, e.g. \"8,6,8\" (must sum to log2 n)")                  \
  X(FFT_TW_PYRAMID, "OZK_FFT_TW_PYRAMID", 1, "0: twiddles from the flat table")                                          \
  X(FFT_PLAN_CACHE, "OZK_FFT_PLAN_CACHE", 1, "0: twiddle tables are built per call")                                     \
  X(FFT_PLAN_CACHE_MB, "OZK_FFT_PLAN_CACHE_MB", 4096, "MiB of cached twiddle tables per device")                         \
  X(QAP_FOLD_SCALE, "OZK_QAP_FOLD_SCALE", 1, "0: the witness map scales in a pass of its own")                           \
  X(BACE_LDS_SLOTS, "OZK_BACE_LDS_SLOTS", 16, "circuit slots kept in LDS, 0..28")

enum Knob {
#define X(id, env, dflt, doc) K_##id,
  OZK_KNOBS(X)
#undef X
  K_COUNT
};
struct KnobInfo {
  const char* env;
  int dflt;
  const char* doc;
};
inline constexpr KnobInfo KNOBS[K_COUNT] = {
#define X(id, env, dflt, doc) {env, dflt, doc},
    OZK_KNOBS(X)
#undef X
};

struct KnobSnapshot {
  bool has[K_COUNT];
  int val[K_COUNT];
  const char* str[K_COUNT];   // KNOB_STRING entries that are set: a copy of the text
  const KnobSnapshot* older;  // replaced snapshots stay reachable
};
inline std::mutex g_knob_mu;                               // held while a snapshot is built and published
inline std::atomic<const KnobSnapshot*> g_knobs{nullptr};  // the snapshot in force

// reads the environment into a new snapshot and publishes it  (g_knob_mu held)
inline const KnobSnapshot* knob_publish() {
  KnobSnapshot* s = new KnobSnapshot();
  for (int k = 0; k < K_COUNT; k++) {
    const char* e = getenv(KNOBS[k].env);
    s->has[k] = e && *e;
    s->val[k] = s->has[k] ? atoi(e) : 0;
    if (s->has[k] && KNOBS[k].dflt == KNOB_STRING) s->str[k] = strdup(e);
  }
  s->older = g_knobs.load(std::memory_order_relaxed);
  g_knobs.store(s, std::memory_order_release);
  return s;
}
inline const KnobSnapshot* knob_snapshot() {
  const KnobSnapshot* s = g_knobs.load(std::memory_order_acquire);
  if (s) return s;
  std::lock_guard<std::mutex> lock(g_knob_mu);
  s = g_knobs.load(std::memory_order_relaxed);
  return s ? s : knob_publish();
}
inline void env_reload() {
  std::lock_guard<std::mutex> lock(g_knob_mu);
  knob_publish();
}

inline int knob_or(Knob k, int computed) {
  const KnobSnapshot* s = knob_snapshot();
  return s->has[k] ? s->val[k] : computed;
}
inline int knob(Knob k) { return knob_or(k, KNOBS[k].dflt); }
inline const char* knob_str(Knob k) { return knob_snapshot()->str[k]; }

}  // namespace ozk
