// k_mix.hip — Mixup / CutMix of the (B, T, H, W) fp32 frame batch in place (mds_mixup, include/mds.h; reference
// src/mixup.py::TimmMixup).  Sample i is combined with sample B - 1 - i, so a thread that owns four columns of a pair reads
// them from both samples, forms both results from the two original values and writes both: no copy of the batch, no second
// pass.  The per-sample jobs (a few bytes each) are kernel arguments.
//
// Roofline: pure HBM streaming.  A blended pair is read once and written once (2 x 4 B per element and direction), a CutMix
// pair moves its box only, a pair without a job is not touched.  No LDS, no atomics; a lane keeps two 16-byte loads in flight.
#include "elem.h"

// the header's arithmetic contract: every product and every sum is rounded on its own (no fused multiply-add)
#pragma clang fp contract(off)

// what a job writes of its own sample, as a box: everything (BLEND), its box (CUT), nothing (NONE, an empty box)
struct MixBox { int yl, yh, xl, xh; };
MDS_DEV MixBox mix_box(const mds_mix_job& jb, int H, int W) {
  MixBox r = {0, 0, 0, 0};
  if (jb.mode == MDS_MIX_BLEND) { r.yh = H; r.xh = W; }
  else if (jb.mode == MDS_MIX_CUT && jb.yl < jb.yh && jb.xl < jb.xh) { r.yl = jb.yl; r.yh = jb.yh; r.xl = jb.xl; r.xh = jb.xh; }
  return r;
}
// bit c of the result: column x + c of row y lies in the box
MDS_DEV unsigned mix_mask(const MixBox& bx, int y, int x) {
  if (y < bx.yl || y >= bx.yh) return 0u;
  int lo = bx.xl - x, hi = bx.xh - x;
  lo = lo < 0 ? 0 : (lo > 4 ? 4 : lo);
  hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
  return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}
MDS_DEV float mix_value(const mds_mix_job& jb, float own, float other) {
  return jb.mode == MDS_MIX_BLEND ? own * jb.lam + other * jb.oml : other;
}

// the smoothed, mixed target rows of this launch's pairs: 2 * npairs * C values, a few threads of one block
MDS_DEV void mix_targets(const mds_mixup_args& a) {
  const int n = 2 * a.npairs * a.C;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int s = e / a.C, c = e - s * a.C, k = s >> 1;
    const bool upper = (s & 1) != 0;
    const int r = upper ? a.B - 1 - (a.pair0 + k) : a.pair0 + k;
    const float lam = upper ? a.hi[k].lam : a.lo[k].lam, oml = upper ? a.hi[k].oml : a.lo[k].oml;
    const float t1 = a.target[(long)r * a.C + c], t2 = a.target[(long)(a.B - 1 - r) * a.C + c];
    const float y1 = (1.0f - t1) * a.off_value + t1 * a.on_value;
    const float y2 = (1.0f - t2) * a.off_value + t2 * a.on_value;
    a.target_out[(long)r * a.C + c] = y1 * lam + y2 * oml;
  }
}

// grid = (blocks of the grid-stride loop, pairs of the launch); one work item = four consecutive columns of one row of one
// plane, inside the bounding box of what the pair's two jobs write
__global__ __launch_bounds__(256) void mixup_kernel(mds_mixup_args a) {
  const int k = blockIdx.y;
  if (blockIdx.x == 0 && k == 0 && a.target) mix_targets(a);
  const mds_mix_job ji = a.lo[k], jj = a.hi[k];
  const int H = a.H, W = a.W;
  const MixBox bi = mix_box(ji, H, W), bj = mix_box(jj, H, W);
  const bool ei = bi.yh == 0, ej = bj.yh == 0;      // (a box that writes something has yh > 0)
  if (ei && ej) return;
  const int y0 = ei ? bj.yl : (ej ? bi.yl : (bi.yl < bj.yl ? bi.yl : bj.yl));
  const int y1 = ei ? bj.yh : (ej ? bi.yh : (bi.yh > bj.yh ? bi.yh : bj.yh));
  const int x0 = ei ? bj.xl : (ej ? bi.xl : (bi.xl < bj.xl ? bi.xl : bj.xl));
  const int x1 = ei ? bj.xh : (ej ? bi.xh : (bi.xh > bj.xh ? bi.xh : bj.xh));
  const unsigned q0 = (unsigned)x0 >> 2, nq = (((unsigned)x1 + 3u) >> 2) - q0, nr = (unsigned)(y1 - y0);
  const unsigned items = (unsigned)a.T * nr * nq;      // < 2^31: T * H * W is
  const long n = (long)a.T * H * W;
  float* xi = a.x + (long)(a.pair0 + k) * n;
  float* xj = a.x + (long)(a.B - 1 - (a.pair0 + k)) * n;
  const bool vec = (W & 3) == 0 && ((uintptr_t)a.x & 15) == 0;      // then every row of every sample starts 16-byte aligned
  for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
    const unsigned row = it / nq, q = it - row * nq, t = row / nr;
    const int y = (int)(row - t * nr) + y0, x = (int)((q0 + q) << 2);
    const unsigned mi = mix_mask(bi, y, x), mj = mix_mask(bj, y, x), need = mi | mj;
    if (!need) continue;
    const long off = ((long)t * H + y) * W + x;
    float va[4] = {0.f, 0.f, 0.f, 0.f}, vb[4] = {0.f, 0.f, 0.f, 0.f}, oi[4], oj[4];
    if (vec && need == 15u) {
      load4(xi + off, va);
      load4(xj + off, vb);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (need >> c & 1u) { va[c] = xi[off + c]; vb[c] = xj[off + c]; }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) { oi[c] = mix_value(ji, va[c], vb[c]); oj[c] = mix_value(jj, vb[c], va[c]); }
    if (vec && mi == 15u) store4(xi + off, oi);
    else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (mi >> c & 1u) xi[off + c] = oi[c];
    }
    if (vec && mj == 15u) store4(xj + off, oj);
    else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (mj >> c & 1u) xj[off + c] = oj[c];
    }
  }
}

extern "C" long mds_mixup(const mds_mixup_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a && a->x, "mixup: null batch");
  MDS_REQUIRE(a->B >= 2 && a->B % 2 == 0, "mixup: B = %d (sample i is paired with sample B - 1 - i: B must be even)", a->B);
  MDS_REQUIRE(a->T > 0 && a->H > 0 && a->W > 0 && (long)a->T * a->H * a->W < 2147483647L, "mixup: T x H x W = %d x %d x %d", a->T, a->H, a->W);
  MDS_REQUIRE(a->npairs >= 1 && a->npairs <= MDS_MIX_MAX_PAIRS, "mixup: npairs = %d (1 .. %d per launch)", a->npairs, MDS_MIX_MAX_PAIRS);
  MDS_REQUIRE(a->pair0 >= 0 && a->pair0 + a->npairs <= a->B / 2, "mixup: pairs %d .. %d of %d", a->pair0, a->pair0 + a->npairs - 1, a->B / 2);
  if (a->target) {
    MDS_REQUIRE(a->target_out && a->C >= 1, "mixup: target needs target_out and C >= 1 (C = %d)", a->C);
    const float* te = a->target + (long)a->B * a->C;
    MDS_REQUIRE(a->target_out >= te || a->target_out + (long)a->B * a->C <= a->target, "mixup: target_out overlaps target");
  }
  long most = 0;      // work items (four columns) of the launch's largest pair
  for (int k = 0; k < a->npairs; ++k) {
    long full = 0, box = 0;
    for (int s = 0; s < 2; ++s) {
      const mds_mix_job& jb = s ? a->hi[k] : a->lo[k];
      MDS_REQUIRE(jb.mode >= MDS_MIX_NONE && jb.mode <= MDS_MIX_CUT, "mixup: mode %d of sample %d", jb.mode, s ? a->B - 1 - (a->pair0 + k) : a->pair0 + k);
      if (jb.mode == MDS_MIX_CUT)
        MDS_REQUIRE(0 <= jb.yl && jb.yl <= jb.yh && jb.yh <= a->H && 0 <= jb.xl && jb.xl <= jb.xh && jb.xh <= a->W,
                    "mixup: box rows [%d, %d) x columns [%d, %d) of a %d x %d frame", jb.yl, jb.yh, jb.xl, jb.xh, a->H, a->W);
      if (jb.mode == MDS_MIX_BLEND) full = 1;
      if (jb.mode == MDS_MIX_CUT) box += (long)(jb.yh - jb.yl) * ((jb.xh - jb.xl + 3) / 4 + 1);
    }
    const long whole = (long)a->H * ((a->W + 3) / 4);
    const long items = (long)a->T * (full || box > whole ? whole : box);
    most = items > most ? items : most;
  }
  if (most == 0 && !a->target) return 0;      // nothing but NONE jobs and empty boxes
  const long cap = mds_knob(MDS_KNOB_STREAM_BLOCKS) ? mds_knob(MDS_KNOB_STREAM_BLOCKS) : 2048;      // as elem.h::stream_blocks
  long bx = (most + 255) / 256;
  bx = bx > cap ? cap : (bx < 1 ? 1 : bx);
  MDS_LAUNCH(mixup_kernel, dim3((unsigned)bx, (unsigned)a->npairs), dim3(256), 0, stream, *a);
  return mds_check_launch("mixup");
}
