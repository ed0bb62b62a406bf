// Host build of the compressed-point codec (octopuszk_amd/csrc/point_codec.cuh): the same header the kernels of
// point_codec.hip compile, so that tests/test_codec_cpu.py checks the roots, codes and bytes the GPU produces.
//   g++ -std=c++17 -O2 -shared -fPIC -o _codec_hostcheck.so codec_hostcheck.cpp
#include "../../octopuszk_amd/csrc/point_codec.cuh"
using namespace ozk;

// a: 8 canonical words -> root (8 words); returns 1 when a is a square
extern "C" int cdhc_fq_sqrt(const u32* a, u32* root) {
  u32 w[8], r[8];
  for (int i = 0; i < 8; i++) w[i] = a[i];
  CdFq y;
  const bool ok = fq_sqrt(codec_fq(w), y);
  from_mont(y, r);
  for (int i = 0; i < 8; i++) root[i] = r[i];
  return ok ? 1 : 0;
}

// a: c0 | c1 (16 words) -> root c0 | c1
extern "C" int cdhc_fq2_sqrt(const u32* a, u32* root) {
  u32 w0[8], w1[8], r0[8], r1[8];
  for (int i = 0; i < 8; i++) {
    w0[i] = a[i];
    w1[i] = a[8 + i];
  }
  CdF2 x, y;
  x.c0 = codec_fq(w0);
  x.c1 = codec_fq(w1);
  const bool ok = fq2_sqrt(x, y);
  from_mont(y.c0, r0);
  from_mont(y.c1, r1);
  for (int i = 0; i < 8; i++) {
    root[i] = r0[i];
    root[8 + i] = r1[i];
  }
  return ok ? 1 : 0;
}

// fmt 0: wire-in (8 words per coordinate), 1: wire-out (16)
extern "C" int cdhc_g1_decode(const u32* in, int fmt, u32* out) {
  CodecG1 p;
  const int code = codec_g1_decode(in, p);
  codec_g1_store(p, fmt ? 16 : 8, out);
  return code;
}
extern "C" int cdhc_g2_decode(const u32* in, int fmt, u32* out) {
  CodecG2 p;
  const int code = codec_g2_decode(in, p);
  codec_g2_store(p, fmt ? 16 : 8, out);
  return code;
}
extern "C" void cdhc_g1_encode(const u32* in, int fmt, u32* out) { codec_g1_encode(in, fmt ? 16 : 8, out); }
extern "C" void cdhc_g2_encode(const u32* in, int fmt, u32* out) { codec_g2_encode(in, fmt ? 16 : 8, out); }
