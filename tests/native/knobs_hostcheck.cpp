// Host build of the knob table (octopuszk_amd/csrc/knobs.h) for tests/test_knobs_cpu.py: plain g++, no HIP.
#include <string.h>

#include <thread>

#include "../../octopuszk_amd/csrc/knobs.h"

using namespace ozk;

extern "C" {
int kh_count() { return K_COUNT; }
int kh_index(const char* env) {
  for (int k = 0; k < K_COUNT; k++)
    if (strcmp(KNOBS[k].env, env) == 0) return k;
  return -1;
}
const char* kh_env(int k) { return KNOBS[k].env; }
const char* kh_doc(int k) { return KNOBS[k].doc; }
int kh_default(int k) { return KNOBS[k].dflt; }
int kh_computed() { return KNOB_COMPUTED; }
int kh_string() { return KNOB_STRING; }
int kh_knob(int k) { return knob((Knob)k); }
int kh_knob_or(int k, int computed) { return knob_or((Knob)k, computed); }
const char* kh_knob_str(int k) { return knob_str((Knob)k); }
void kh_reload() { env_reload(); }
// the value a thread started NOW reads
int kh_knob_in_new_thread(int k) {
  int v = 0;
  std::thread t([&] { v = knob((Knob)k); });
  t.join();
  return v;
}
}
