// Stand-alone race check of the knob table (octopuszk_amd/csrc/knobs.h), built with -fsanitize=thread by
// tests/test_knobs_cpu.py and run as a program of its own: eight readers hammer knob() / knob_or() / knob_str() while
// one thread alternates setenv and env_reload().  Every value a reader sees must be one of the two published ones.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../octopuszk_amd/csrc/knobs.h"

using namespace ozk;

int main() {
  setenv("OZK_MSM_FIN_MAX", "7", 1);
  setenv("OZK_FFT_KS", "8,6,8", 1);
  if (knob(K_MSM_FIN_MAX) != 7) return 2;   // the first snapshot, before anybody else runs (getenv beside setenv is a
                                            // race of the C library's, not of the table's)
  std::atomic<bool> stop{false};
  std::atomic<long> bad{0}, reads{0};
  std::vector<std::thread> readers;
  for (int t = 0; t < 8; t++)
    readers.emplace_back([&] {
      long n = 0;
      while (!stop.load(std::memory_order_relaxed)) {
        const int a = knob(K_MSM_FIN_MAX), b = knob_or(K_MSM_C, 13), g = knob(K_MSM_GLV);
        const char* s = knob_str(K_FFT_KS);
        if ((a != 7 && a != 9) || (b != 13 && b != 5) || g != 1 || !s || (strcmp(s, "8,6,8") && strcmp(s, "7,7,8"))) bad++;
        n++;
      }
      reads += n;
    });
  for (int i = 0; i < 4000; i++) {
    const bool odd = i & 1;
    setenv("OZK_MSM_FIN_MAX", odd ? "7" : "9", 1);
    setenv("OZK_FFT_KS", odd ? "8,6,8" : "7,7,8", 1);
    if (odd) unsetenv("OZK_MSM_C");
    else setenv("OZK_MSM_C", "5", 1);
    env_reload();
  }
  stop = true;
  for (auto& t : readers) t.join();
  printf("reads %ld bad %ld\n", reads.load(), bad.load());
  return bad.load() ? 1 : 0;
}
