// k_rng.hip - the engine's own random stream for the DropPath / dropout masks (mds_mask_fill, include/mds.h).
// Philox4x32-10 is counter based: element e of the mask arena is a pure function of (seed, stream, draw, e), so the launch
// keeps no state, needs no ordering between its threads, and a host implementation of the header's definition predicts every
// bit.  One thread computes one output block of the generator = four consecutive elements: ten rounds of two 32 x 32 -> 64-bit
// multiplies, one 16-byte load of keep[], one 16-byte store.  The arena of a training plan is a few thousand floats (config 2:
// one or a few workgroups), so this is a launch-latency kernel: nothing to tile, nothing to share.
#include "elem.h"
#include <cstring>
#include <vector>

MDS_DEV void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;      // (the bump after the tenth round is dead)
  }
}

MDS_DEV float mask_value(uint32_t r, float keep) {
  const float u = (float)(r >> 8) * 5.9604644775390625e-8f;      // 24 bits * 2^-24: exact, 0 <= u < 1
  return u < keep ? 1.0f / keep : 0.0f;
}

__global__ __launch_bounds__(256) void mask_fill_kernel(mds_mask_fill_args a) {
  const long blk = (long)blockIdx.x * 256 + threadIdx.x, e0 = blk * 4;      // this thread's output block / its first element
  if (e0 >= a.n) return;
  uint32_t c[4] = {(uint32_t)blk, a.stream, (uint32_t)a.draw, (uint32_t)(a.draw >> 32)};
  philox4x32_10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
  if (e0 + 4 <= a.n) {
    const f32x4 kp = *(const f32x4*)(a.keep + e0);
    const f32x4 m = {mask_value(c[0], kp[0]), mask_value(c[1], kp[1]), mask_value(c[2], kp[2]), mask_value(c[3], kp[3])};
    *(f32x4*)(a.mask + e0) = m;
  } else {      // the arena's last, partial block (n % 4 elements)
    for (int j = 0; e0 + j < a.n; ++j) a.mask[e0 + j] = mask_value(c[j], a.keep[e0 + j]);
  }
}

// keep[] lives in device memory.  The product's mds_platform_hw.h copies it to the host (blocking); a platform whose header
// offers no mds_read_back has its buffers in host memory and lands here
template <typename... S> static inline int mds_read_back(void* dst, const void* src, size_t bytes, S...) {
  std::memcpy(dst, src, bytes);
  return 0;
}

extern "C" long mds_mask_fill(const mds_mask_fill_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a && a->mask && a->keep, "mask_fill: null mask / keep");
  MDS_REQUIRE(a->n > 0 && a->n < 2147483647L, "mask_fill: n = %ld", a->n);
  MDS_REQUIRE(((uintptr_t)a->mask & 15) == 0 && ((uintptr_t)a->keep & 15) == 0, "mask_fill: mask and keep must be 16-byte aligned");
  if (!a->keep_checked) {
    std::vector<float> kp((size_t)a->n);
    MDS_REQUIRE(mds_read_back(kp.data(), a->keep, sizeof(float) * (size_t)a->n, (hipStream_t)stream) == 0, "mask_fill: reading keep[] back failed");
    for (long e = 0; e < a->n; ++e)
      MDS_REQUIRE(kp[e] > 0.0f && kp[e] <= 1.0f, "mask_fill: keep[%ld] = %g is outside (0, 1]", e, (double)kp[e]);
  }
  MDS_LAUNCH(mask_fill_kernel, dim3((unsigned)cdiv(cdiv(a->n, 4), 256)), dim3(256), 0, stream, *a);
  return mds_check_launch("mask_fill");
}
