// se_tail.h — squeeze-excite tail of the pooling depthwise kernels (mds_se_tail_t; k_dw.hip, k_dwx.hip).
//
// The launch that completes pool[n] also turns it into gate[n] = sigmoid(W2 silu(W1 pool[n] + b1) + b2): the block that
// finishes an image LAST runs the two products before it exits.  "Last" is a per-image ticket counted in strips (tiles):
//   1. every lane waits for the acknowledgements of its pool atomics (fp64 atomicAdd: device scope, performed at the
//      coherence point behind the XCDs' L2s - the same place the ticket lives), then the block barrier;
//   2. one thread adds the block's strip count of the image to ticket[n] (device-scope atomic, returns the old value);
//      the add that completes strips-per-image x channel chunks is ordered after every other block's step 1, i.e. after
//      every partial of pool[n] - and resets the ticket for the next launch;
//   3. that block reads pool[n] with device-scope loads (never a line its own L1 / L2 may hold from before) and runs the tail.
// The arithmetic is fp32 in the operation order of se_fc_fwd_kernel (k_misc.hip): a hidden value is one wave's sum over
// lanes that each own 16-byte chunks lane, lane + 64, ... of the channel axis; a gate value is b2 + the R products in r
// order.  Only the number of rows whose loads are in flight together differs (RH: the register budget of the host kernel).
#pragma once
#include "elem.h"

// two consecutive doubles of a pooled row that other workgroups of this launch accumulated with device-scope atomics: the
// device-scope 8-byte loads of ld_coherent4 (the split-K partials' path), the 16 bytes reinterpreted
MDS_DEV f64x2 se_ld_pool2(const double* p) {
  const f32x4 r = ld_coherent4((const float*)p);
  return __builtin_bit_cast(f64x2, r);
}

#define SE_TAIL_JU 5   // 16-byte chunks per lane: C <= 4 * 64 * SE_TAIL_JU = MDS_SE_TAIL_CMAX
static_assert(4 * 64 * SE_TAIL_JU == MDS_SE_TAIL_CMAX, "the tail keeps a whole pooled row in registers");

// gate row of image group `grp` from its COMPLETED pooled row; called by all 256 threads of the block
template <int RH>
MDS_DEV void se_tail_group(const mds_se_tail_t& se, const double* pool, int C, int grp) {
  __shared__ float se_hid[MDS_SE_TAIL_RMAX], se_act[MDS_SE_TAIL_RMAX];
  constexpr int JU = SE_TAIL_JU;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, R = se.R, C4 = C >> 2;
  const double* v = pool + (long)grp * C;
  f32x4 vv[JU];
  int fo[JU];
#pragma unroll
  for (int j = 0; j < JU; ++j) {
    const int f = lane + 64 * j;
    fo[j] = f < C4 ? 4 * f : 0;
    const f64x2 pa = se_ld_pool2(v + fo[j]), pb = se_ld_pool2(v + fo[j] + 2);
    vv[j] = (f32x4){(float)pa[0], (float)pa[1], (float)pb[0], (float)pb[1]};
    if (f >= C4) vv[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  // hidden: wave k owns rows k, k + 4, ...; RH rows' loads are issued before the first product
  for (int k0 = 0; 4 * k0 < R; k0 += RH) {
    f32x4 wv[RH][JU];
#pragma unroll
    for (int rr = 0; rr < RH; ++rr) {
      const int r = wave + 4 * (k0 + rr);
      const float* wr = se.w1 + (long)(r < R ? r : R - 1) * C;
#pragma unroll
      for (int j = 0; j < JU; ++j) wv[rr][j] = *(const f32x4*)(wr + fo[j]);
    }
#pragma unroll
    for (int rr = 0; rr < RH; ++rr) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < JU; ++j) {
        const f32x4 p = wv[rr][j] * vv[j];
        acc += (p[0] + p[1]) + (p[2] + p[3]);
      }
      const float s = wave_sum(acc);
      const int r = wave + 4 * (k0 + rr);
      if (lane == 0 && r < R) se_hid[r] = s;
    }
  }
  __syncthreads();
  if (tid < R) {
    const float h = se_hid[tid] + se.b1[tid];
    se_act[tid] = siluf_(h);
    se.hidden[(long)grp * R + tid] = h;
  }
  __syncthreads();
  // gate: a thread owns the 16-byte channel chunks tid and tid + 256 (C4 <= 320); 2 * RH rows of w2t in flight per chunk
  {
    constexpr int RB = 2 * RH;
    const int f0 = tid, f1 = tid + 256;
    const bool ok0 = f0 < C4, ok1 = f1 < C4;
    const int o0 = ok0 ? 4 * f0 : 0, o1 = ok1 ? 4 * f1 : 0;
    f32x4 s0 = *(const f32x4*)(se.b2 + o0), s1 = *(const f32x4*)(se.b2 + o1);
    for (int r0 = 0; r0 < R; r0 += RB) {
      f32x4 w0[RB], w1[RB];
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        const float* wr = se.w2t + (long)(r0 + rr < R ? r0 + rr : R - 1) * C;
        w0[rr] = *(const f32x4*)(wr + o0);
        w1[rr] = *(const f32x4*)(wr + o1);
      }
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        if (r0 + rr < R) {   // (block-uniform)
          const float av = se_act[r0 + rr];
          s0 += w0[rr] * av;
          s1 += w1[rr] * av;
        }
      }
    }
    float* grow = se.gate + (long)grp * C;
    if (ok0) *(f32x4*)(grow + o0) = (f32x4){sigmoidf_(s0[0]), sigmoidf_(s0[1]), sigmoidf_(s0[2]), sigmoidf_(s0[3])};
    if (ok1) *(f32x4*)(grow + o1) = (f32x4){sigmoidf_(s1[0]), sigmoidf_(s1[1]), sigmoidf_(s1[2]), sigmoidf_(s1[3])};
  }
  __syncthreads();   // se_hid / se_act are written again by the block's next group
}

// Steps 1-3 for a block whose (up to 8) flushed strips belong to the images img_s[0..7] (-1: no strip; non-decreasing):
// `per_image` = strips per image x channel chunks of the launch.  Called by all 256 threads after the pool atomics.
template <int RH>
MDS_DEV void se_tail_tickets(const mds_se_tail_t& se, const double* pool, int C, const int* img_s, int per_image) {
  __shared__ int se_last[8], se_nlast;
  wait_vm<0>();      // this lane's pool atomics are acknowledged (explicit: a workgroup barrier alone does not wait for them)
  __syncthreads();
  if (threadIdx.x == 0) {
    int nl = 0, cur = -1, k = 0;
    for (int s = 0; s <= 8; ++s) {
      const int n = s < 8 ? img_s[s] : -1;
      if (n == cur && n >= 0) { ++k; continue; }
      if (cur >= 0) {
        const int t = atomicAdd(se.ticket + cur, k);
        if (t + k == per_image) {
          atomicExch(se.ticket + cur, 0);   // ready for the next launch
          se_last[nl++] = cur;
        }
      }
      cur = n; k = 1;
    }
    se_nlast = nl;
  }
  __syncthreads();
  const int nl = se_nlast;
  for (int i = 0; i < nl; ++i) se_tail_group<RH>(se, pool, C, se_last[i]);
}

// host side: what every kernel with the tail asks of its arguments (MDS_REQUIRE returns from the caller)
#define SE_TAIL_REQUIRE(a, what)                                                                                            \
  do {                                                                                                                      \
    const mds_se_tail_t& se_ = (a)->se;                                                                                     \
    MDS_REQUIRE((a)->pool, what ": the squeeze-excite tail needs pool");                                                    \
    MDS_REQUIRE((a)->epi.mode != MDS_EPI_NONE, what ": the squeeze-excite tail needs an output transform (epi)");          \
    MDS_REQUIRE(se_.w2t, what ": the squeeze-excite tail needs w2t (MDS_PACK_IO_F32)");                                     \
    MDS_REQUIRE(se_.w1 && se_.b1 && se_.b2 && se_.hidden && se_.ticket, what ": squeeze-excite tail: null pointer");       \
    MDS_REQUIRE(se_.R > 0 && se_.R <= MDS_SE_TAIL_RMAX, what ": squeeze-excite tail: R must be 1 .. %d", MDS_SE_TAIL_RMAX); \
    MDS_REQUIRE((a)->C % 4 == 0 && (a)->C <= MDS_SE_TAIL_CMAX, what ": squeeze-excite tail: C %% 4 == 0 and C <= %d",       \
                MDS_SE_TAIL_CMAX);                                                                                          \
    MDS_REQUIRE((((uintptr_t)(a)->pool | (uintptr_t)se_.w1 | (uintptr_t)se_.w2t | (uintptr_t)se_.b2 |                       \
                  (uintptr_t)se_.gate) & 15) == 0,                                                                          \
                what ": squeeze-excite tail: pool / w1 / w2t / b2 / gate must be 16-byte aligned (16-byte vector accesses)"); \
  } while (0)
