// k_det.hip - the finishing kernel of the deterministic way out (mds_partial_t / mds_wgrad_finish, include/mds.h).
// The producers (weight-gradient kernels, GeM's dp, the loss value) leave one slot per block in a caller-owned fp32 buffer;
// this kernel adds the slots in an order that depends on the slot COUNT and the result's SIZE only and accumulates the sum into
// the result:   result[e] += (((S0 + S1) + S2) + ...) + S(G-1),   Sg = slots [g * per, (g + 1) * per) added first to last,
// per = ceil(slots / G).  A lane owns one 16-byte column of the slots with four slots' loads in flight; a block is G slot ranges
// x 256 / G columns and the range sums meet in LDS.  G = 4 for the large results (blocks.2.1: 256 slots x 82 944 floats, 85 MB: a
// streaming reduce, 324 blocks), 16 / 64 for the small ones - a depthwise filter, the stem or GeM's exponent is a few thousand floats
// in hundreds of slots, and with G = 4 a handful of blocks would each walk a hundred slots one memory round trip after the other
// on the dependent chain.
#include "elem.h"

template <int G, bool VEC>      // VEC: the result is 16-byte aligned (one 16-byte read-modify-write per lane); else element by element
__global__ __launch_bounds__(256) void wgrad_finish_kernel(mds_wgrad_finish_args a) {
  constexpr int CPB = 256 / G;      // columns per block
  __shared__ f32x4 red[G - 1][CPB];
  const int c = threadIdx.x % CPB, grp = threadIdx.x / CPB;
  const long col = ((long)blockIdx.x * CPB + c) * 4;      // first element of this lane's column
  const long per = (a.slots + G - 1) / G;
  const long s0 = grp * per, s1 = s0 + per < a.slots ? s0 + per : a.slots;
  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  if (col < a.numel) {      // (slot_stride is numel rounded up to 4: a column that starts inside numel ends inside the slot)
    const float* p = a.partial + s0 * a.slot_stride + col;
    long s = s0;
    for (; s + 4 <= s1; s += 4, p += 4 * a.slot_stride) {
      const f32x4 v0 = *(const f32x4*)p, v1 = *(const f32x4*)(p + a.slot_stride), v2 = *(const f32x4*)(p + 2 * a.slot_stride),
                  v3 = *(const f32x4*)(p + 3 * a.slot_stride);
      sum += v0; sum += v1; sum += v2; sum += v3;
    }
    for (; s < s1; ++s, p += a.slot_stride) sum += *(const f32x4*)p;
  }
  if (grp > 0) red[grp - 1][c] = sum;
  __syncthreads();
  if (grp == 0 && col < a.numel) {
    for (int g = 0; g < G - 1; ++g) sum += red[g][c];
    float* d = a.dst + col;
    if (VEC) {
      *(f32x4*)d = *(const f32x4*)d + sum;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (col + j < a.numel) d[j] += sum[j];
    }
  }
}

extern "C" long mds_wgrad_finish(const mds_wgrad_finish_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a && a->partial && a->dst && a->numel > 0 && a->slots > 0, "wgrad_finish: bad args");
  MDS_REQUIRE(a->slot_stride >= a->numel && a->slot_stride % 4 == 0 && ((uintptr_t)a->partial & 15) == 0, "wgrad_finish: slot_stride %% 4, 16-byte aligned partial");
  MDS_REQUIRE(a->numel < 2147483647L, "wgrad_finish: numel");
  const bool vec = ((uintptr_t)a->dst & 15) == 0 && a->numel % 4 == 0;
  const dim3 block(256);
#define FIN_GO(G) do { const dim3 grid((unsigned)cdiv(a->numel, 4 * (256 / G))); \
    if (vec) MDS_LAUNCH((wgrad_finish_kernel<G, true>), grid, block, 0, stream, *a); \
    else MDS_LAUNCH((wgrad_finish_kernel<G, false>), grid, block, 0, stream, *a); } while (0)
  if (a->numel >= MDS_FINISH_WIDE) FIN_GO(MDS_FINISH_GROUPS);
  else if (a->numel >= MDS_FINISH_MID) FIN_GO(MDS_FINISH_GROUPS_MID);
  else FIN_GO(MDS_FINISH_GROUPS_SMALL);
#undef FIN_GO
  return mds_check_launch("wgrad_finish");
}

int wg_finish(const mds_partial_t& pt, float* result, long numel, long slots, mds_stream_t stream) {
  if (!pt.buf) return 0;
  mds_wgrad_finish_args f = {pt.buf, result, numel, slots, (numel + 3) & ~3L};
  return (int)mds_wgrad_finish(&f, stream);
}
