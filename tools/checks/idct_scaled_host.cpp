// idct_scaled_host.cpp — csrc/ldt_idct_scaled.hpp compiled for the host, for
// tests/test_idct_scaled_ops.py: the reduced inverse DCTs of a drafted decode
// as k_idct_scaled runs them, callable through ctypes on numpy arrays and
// compared there with Pillow's draft() (zero mismatches allowed).
//
//   g++ -std=c++17 -O2 -shared -fPIC idct_scaled_host.cpp -o libidct_scaled_host.so
//
// With -DIDCT_SCALED_HOST_MAIN it is a stand-alone program instead (build it
// with -fsanitize=address,undefined): the three transforms on extreme blocks
// (coefficients of +-2047 and the int16 limits times quantisers 1, 255 and
// 65535, in every position the transforms read and in all of them at once); it
// checks that flat blocks give the sample libjpeg's shortcut gives and prints
// "idct scaled ok".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../lance-distributed-training_amd/csrc/ldt_idct_scaled.hpp"

using namespace ldt;

// One block: coefficients and quantisers in natural (row-major) order, `sc` in
// {4, 2, 1}; out: sc x sc samples, row-major. Dequantised as k_idct does
// (int16 coefficient times uint16 quantiser, mod 2^32).
static void block(const int16_t *coef, const uint16_t *q, int sc, uint8_t *out) {
  int32_t blk[64];
  for (int i = 0; i < 64; ++i) blk[i] = (int32_t)((uint32_t)(int32_t)coef[i] * (uint32_t)q[i]);
  if (sc == 4) idct_4x4(blk, out);
  else if (sc == 2) idct_2x2(blk, out);
  else out[0] = idct_1x1(blk[0]);
}

extern "C" {

// coef: bw * bh blocks (block (bx, by) at by * bw + bx) of 64 int16 each, q: 64
// quantisers; plane: bh * sc rows of bw * sc bytes.
void idct_scaled_host_plane(const int16_t *coef, const uint16_t *q, int bw, int bh, int sc, uint8_t *plane) {
  for (int by = 0; by < bh; ++by)
    for (int bx = 0; bx < bw; ++bx) {
      uint8_t o[16];
      block(coef + 64 * ((int64_t)by * bw + bx), q, sc, o);
      for (int r = 0; r < sc; ++r)
        memcpy(plane + ((int64_t)(by * sc + r) * bw + bx) * sc, o + sc * r, (size_t)sc);
    }
}

} // extern "C"

#ifdef IDCT_SCALED_HOST_MAIN
int main() {
  const int16_t cvals[] = {0, 1, -1, 2047, -2047, 1023, -1024, 32767, -32768};
  const uint16_t qvals[] = {1, 2, 16, 255, 256, 32767, 65535};
  uint8_t o[16];
  uint64_t sum = 0;
  for (uint16_t qv : qvals) {
    uint16_t q[64];
    for (int i = 0; i < 64; ++i) q[i] = qv;
    for (int16_t cv : cvals) {
      int16_t coef[64];
      // every coefficient at once, alternating signs, and each position alone
      for (int pat = 0; pat < 66; ++pat) {
        for (int i = 0; i < 64; ++i)
          coef[i] = pat == 0 ? cv : pat == 1 ? (int16_t)(((i ^ (i >> 3)) & 1) ? cv : (cv == -32768 ? 32767 : -cv))
                                             : (i == pat - 2 ? cv : 0);
        for (int sc = 4; sc >= 1; sc >>= 1) {
          block(coef, q, sc, o);
          for (int i = 0; i < sc * sc; ++i) sum += o[i];
        }
      }
    }
  }
  // a flat block (DC only) gives range_limit(DESCALE(dc * q0, 3)) at every scale
  // (the table's index is masked to 10 bits: values past +-512 wrap, as libjpeg's do)
  for (int dc = -512; dc <= 511; ++dc) {
    int16_t coef[64] = {(int16_t)dc};
    uint16_t q[64];
    for (int i = 0; i < 64; ++i) q[i] = 8;
    const int want = dc + 128 < 0 ? 0 : (dc + 128 > 255 ? 255 : dc + 128);
    for (int sc = 4; sc >= 1; sc >>= 1) {
      block(coef, q, sc, o);
      for (int i = 0; i < sc * sc; ++i)
        if (o[i] != want) {
          fprintf(stderr, "idct_scaled_host: flat block dc=%d scale %d gives %d, not %d\n", dc, sc, o[i], want);
          return 1;
        }
    }
  }
  printf("idct scaled ok %llu\n", (unsigned long long)sum);
  return 0;
}
#endif
