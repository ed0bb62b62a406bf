// Host check of octopuszk_amd/csrc/sha256.cuh (tests/test_plonk_batch_cpu.py): the streaming SHA-256 the batched PLONK
// verifier runs one lane per proof, compiled for the host and run directly.
//   stdin:  lines "<mode> <hex of the message>" (an empty message is "-"); mode b absorbs byte by byte, w absorbs
//           as many whole little-endian words as fit after a prefix of `mode digit` bytes (w0 .. w3) and the rest as
//           bytes, s splits the message in three absorb() calls
//   stdout: one line of 64 hex digits per input line
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../octopuszk_amd/csrc/sha256.cuh"

using namespace ozk;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return out;
}

int main() {
  std::string mode, hex;
  while (std::cin >> mode >> hex) {
    const std::vector<uint8_t> msg = unhex(hex);
    uint32_t block[16];
    memset(block, 0xA5, sizeof block);            // the buffer is the caller's and starts as garbage
    Sha256 H;
    H.init(block);
    if (mode == "b") {
      H.absorb(msg.data(), msg.size());
    } else if (mode == "s") {
      const size_t a = msg.size() / 3, b = msg.size() / 2;
      H.absorb(msg.data(), a);
      H.absorb(msg.data() + a, b - a);
      H.absorb(msg.data() + b, msg.size() - b);
    } else {
      size_t at = (size_t)(mode[1] - '0');
      if (at > msg.size()) at = msg.size();
      H.absorb(msg.data(), at);
      std::vector<uint32_t> words;
      for (; at + 4 <= msg.size(); at += 4)
        words.push_back((uint32_t)msg[at] | (uint32_t)msg[at + 1] << 8 | (uint32_t)msg[at + 2] << 16 | (uint32_t)msg[at + 3] << 24);
      H.absorb_le_words(words.data(), (int)words.size());
      H.absorb(msg.data() + at, msg.size() - at);
    }
    uint32_t d[8];
    H.finish(d);
    uint8_t out[32];
    sha256_digest_bytes(d, out);
    for (int i = 0; i < 32; i++) printf("%02x", out[i]);
    printf("\n");
  }
  return 0;
}
