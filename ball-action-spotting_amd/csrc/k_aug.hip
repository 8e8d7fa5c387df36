// k_aug.hip — SURVEY 8(f) N3: the reference's GPU augmentation pipeline (src/ball_action/augmentations.py:7-22,
// src/augmentations.py:42-78) as fused passes over the fp32 frame batch.  See include/mds.h (mds_aug_pass).
//
// Roofline: pure HBM streaming — a sample without spatial filter is read once (bilinear gathers of a near-identity affine
// map: neighbouring lanes touch neighbouring source pixels, the re-use is served by L1/L2) and written once, 4 pixels
// (16 bytes) per lane; algorithmic bytes = 2 x 4 B per pixel (+ the same again per extra filter pass of a sample).  With a raw
// uint8 source (mds_aug_raw_t: the reference's frames processor, src/frames.py, folded into a sample's first pass) that pass
// reads 1 B per source pixel instead of 4; mds_pad_normalize is the same conversion as a stand-alone 1 B in / 4 B out stream.
#include "elem.h"

// Philox-4x32-10 (Salmon et al., SC'11): counter = element index / 4, key = the job's seed
MDS_DEV void philox4(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
  uint32_t c[4] = {c0, c1, 0u, 0u};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = c[j];
}
MDS_DEV void normal4(uint32_t seed, unsigned long long quad, float (&z)[4]) {
  uint32_t r[4];
  philox4((uint32_t)quad, (uint32_t)(quad >> 32), seed, 0x5bd1e995u, r);
  // Box-Muller on two pairs of uniforms in (0, 1]
  const float u0 = ((float)(r[0] >> 8) + 1.0f) * (1.0f / 16777216.0f), u1 = (float)(r[1] >> 8) * (1.0f / 16777216.0f);
  const float u2 = ((float)(r[2] >> 8) + 1.0f) * (1.0f / 16777216.0f), u3 = (float)(r[3] >> 8) * (1.0f / 16777216.0f);
  const float ra = sqrtf(-2.0f * logf(u0)), rb = sqrtf(-2.0f * logf(u2));
  z[0] = ra * cosf(6.28318530718f * u1); z[1] = ra * sinf(6.28318530718f * u1);
  z[2] = rb * cosf(6.28318530718f * u3); z[3] = rb * sinf(6.28318530718f * u3);
}

// One block = one output tile of AUG_TR rows x AUG_TC columns of one frame; one thread = 4 consecutive pixels (one 16-byte store).
// WARP / SHARP / TAPS first stage the SOURCE box the tile needs (the affine image of the tile, or the tile plus its halo) in
// LDS with coalesced row reads - zeros outside the frame, which is exactly the padding all three stages use - and gather
// from there: a direct gather costs 4...48 scalar global loads per pixel (1.1-1.7 TB/s for a rotation, 0.45 TB/s for the
// motion blur, measured), the staged form one 16-byte load per 4 source pixels.  A source box that does not fit (a map far
// from the identity) falls back to direct gathers.
#define AUG_TR 8
#define AUG_TC 128
#define AUG_LDS_FLOATS 7168      // 28 KiB: e.g. 40 rows x 176 columns

MDS_DEV float px(const float* plane, int H, int W, int x, int y) {   // zeros outside, branch-free (clamped address, masked value)
  const bool in = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
  const int xc = x < 0 ? 0 : (x >= W ? W - 1 : x), yc = y < 0 ? 0 : (y >= H ? H - 1 : y);
  const float v = plane[(long)yc * W + xc];
  return in ? v : 0.0f;
}

// ---- the raw uint8 source (mds_aug_raw_t / mds_pad_normalize): one plane of (sh, sw) bytes placed at (pt, pl) of the H x W frame.
// The header's conversion is ONE correctly rounded fp32 division - what torch computes for .to(float32) / 255.0; a multiply by
// 1.0f / 255 rounds 126 of the 256 byte values differently.
MDS_DEV float u8_unit(unsigned byte) { return (float)byte / 255.0f; }
struct RawPlane { const unsigned char* p; int sh, sw, pt, pl; float fillv; };
// frame pixels (gx .. gx + 3, gy), gy inside the frame: converted bytes inside the source rectangle, the converted fill in the
// pad band, zeros beyond the frame's columns.  Four bytes in one load where the group lies inside the source row at a 4-byte
// aligned address (source row start, pad_left and src_w decide that), bytes otherwise.
MDS_DEV f32x4 raw_quad(const RawPlane& s, int W, int gx, int gy) {
  const int ry = gy - s.pt, rx = gx - s.pl;
  f32x4 v;
  if ((unsigned)ry < (unsigned)s.sh) {
    const unsigned char* p = s.p + (long)ry * s.sw + rx;
    if (rx >= 0 && rx + 3 < s.sw && ((uintptr_t)p & 3) == 0) {
      const uint32_t w = *(const uint32_t*)p;
      return (f32x4){u8_unit(w & 255u), u8_unit((w >> 8) & 255u), u8_unit((w >> 16) & 255u), u8_unit(w >> 24)};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float e = 0.0f;
      if ((unsigned)(gx + j) < (unsigned)W) e = (unsigned)(rx + j) < (unsigned)s.sw ? u8_unit(p[j]) : s.fillv;
      v[j] = e;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (unsigned)(gx + j) < (unsigned)W ? s.fillv : 0.0f;
  }
  return v;
}
MDS_DEV float raw_px(const RawPlane& s, int H, int W, int x, int y) {   // as px(): zeros outside the frame, clamped address, masked value
  const bool in = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
  const int rx = x - s.pl, ry = y - s.pt;
  const bool rect = (unsigned)rx < (unsigned)s.sw && (unsigned)ry < (unsigned)s.sh;
  const int xc = rx < 0 ? 0 : (rx >= s.sw ? s.sw - 1 : rx), yc = ry < 0 ? 0 : (ry >= s.sh ? s.sh - 1 : ry);
  const float v = u8_unit(s.p[(long)yc * s.sw + xc]);
  return in ? (rect ? v : s.fillv) : 0.0f;
}

__global__ __launch_bounds__(256) void aug_kernel(mds_aug_args a) {
  __shared__ float tile[AUG_LDS_FLOATS];
  const int b = blockIdx.z, t = blockIdx.y;
  const mds_aug_job& jb = a.jobs[b];
  if (!jb.active) return;
  const int H = a.H, W = a.W, tiles_x = (W + AUG_TC - 1) / AUG_TC;
  const int ty0 = (int)(blockIdx.x / tiles_x) * AUG_TR, tx0 = (int)(blockIdx.x % tiles_x) * AUG_TC;
  const long plane_off = ((long)b * a.T + t) * H * W;
  // a job with src 0 reads the raw uint8 batch where the launch has one: converted where it is loaded (staging loop, COPY, the
  // direct gathers), fp32 from there on
  const bool raw = a.raw.u8 != nullptr && jb.src == 0;
  const RawPlane rs = {raw ? a.raw.u8 + ((long)b * a.T + t) * a.raw.src_h * a.raw.src_w : nullptr, a.raw.src_h, a.raw.src_w,
                       a.raw.pad_top, a.raw.pad_left, u8_unit((unsigned)a.raw.fill)};
  const float* src = raw ? nullptr : a.buf[jb.src] + plane_off;
  float* dst = a.buf[jb.dst] + plane_off;
  const int mode = jb.mode, tid = threadIdx.x;
  const int y = ty0 + (tid >> 5), x0 = tx0 + 4 * (tid & 31);
  float m[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  // ---- the source box of this tile: [bx0, bx0 + bw) x [by0, by0 + bh)
  int bx0 = tx0, by0 = ty0, bw = 0, bh = 0;
  if (mode == MDS_AUG_WARP) {
#pragma unroll
    for (int j = 0; j < 6; ++j) m[j] = a.maps[((long)b * a.T + t) * 6 + j];
    const float xa = (float)tx0, xb = (float)(tx0 + AUG_TC - 1 < W - 1 ? tx0 + AUG_TC - 1 : W - 1);
    const float ya = (float)ty0, yb = (float)(ty0 + AUG_TR - 1 < H - 1 ? ty0 + AUG_TR - 1 : H - 1);
    float sxl = 1e30f, sxh = -1e30f, syl = 1e30f, syh = -1e30f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float cx = (c & 1) ? xb : xa, cy = (c & 2) ? yb : ya;
      const float sx = m[0] * cx + m[1] * cy + m[2], sy = m[3] * cx + m[4] * cy + m[5];
      sxl = fminf(sxl, sx); sxh = fmaxf(sxh, sx); syl = fminf(syl, sy); syh = fmaxf(syh, sy);
    }
    // clamp to a band around the frame (everything beyond contributes zeros anyway) so the int conversions stay defined
    sxl = fmaxf(sxl, -2.0f); syl = fmaxf(syl, -2.0f); sxh = fminf(sxh, (float)W + 1.0f); syh = fminf(syh, (float)H + 1.0f);
    bx0 = ((int)floorf(sxl)) & ~3; by0 = (int)floorf(syl);
    bw = (int)floorf(sxh) + 2 - bx0; bh = (int)floorf(syh) + 2 - by0;
  } else if (mode == MDS_AUG_SHARP) {
    bx0 = tx0 - 4; by0 = ty0 - 1; bw = AUG_TC + 8; bh = AUG_TR + 2;
  } else if (mode == MDS_AUG_TAPS) {
    bx0 = tx0 - 8; by0 = ty0 - 5; bw = AUG_TC + 16; bh = AUG_TR + 10;      // motion kernel: |dx|, |dy| <= 5 (11 x 11)
  }
  bw = (bw + 3) & ~3;
  bool staged = mode != MDS_AUG_COPY && bw > 0 && bh > 0 && (long)bw * bh <= AUG_LDS_FLOATS;
  if (mode == MDS_AUG_TAPS) {      // taps beyond the staged halo (a larger kernel than 11 x 11): direct gathers
    for (int k = 0; k < jb.ntaps; ++k) staged = staged && jb.tap_dx[k] >= -8 && jb.tap_dx[k] <= 8 && jb.tap_dy[k] >= -5 && jb.tap_dy[k] <= 5;
  }
  __shared__ float tapw[MDS_AUG_MAX_TAPS];
  __shared__ int tapo[MDS_AUG_MAX_TAPS];
  const int ntaps = mode == MDS_AUG_TAPS ? jb.ntaps : 0;
  if (staged && tid < ntaps) { tapw[tid] = jb.tap_w[tid]; tapo[tid] = jb.tap_dy[tid] * bw + jb.tap_dx[tid]; }   // (read once, not per pixel and tap)
  if (staged) {
    const int nq = (bw >> 2) * bh;
    const bool vec = (W & 3) == 0;           // rows start 16-byte aligned and bx0 is a multiple of 4
    for (int e = tid; e < nq; e += 256) {
      const int r = e / (bw >> 2), c4 = (e - r * (bw >> 2)) << 2;
      const int gy = by0 + r, gx = bx0 + c4;
      f32x4 v4 = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)gy < (unsigned)H) {
        if (raw) v4 = raw_quad(rs, W, gx, gy);
        else if (vec && gx >= 0 && gx + 3 < W) v4 = *(const f32x4*)(src + (long)gy * W + gx);
        else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v4[j] = (unsigned)(gx + j) < (unsigned)W ? src[(long)gy * W + gx + j] : 0.f;
        }
      }
      *(f32x4*)(tile + r * bw + c4) = v4;
    }
    __syncthreads();
  }
  if (y >= H || x0 >= W) return;
  auto tap = [&](int gx, int gy) -> float {    // source pixel (gx, gy), zeros outside the frame
    if (staged) {
      const int lx = gx - bx0, ly = gy - by0;
      return ((unsigned)lx < (unsigned)bw && (unsigned)ly < (unsigned)bh) ? tile[ly * bw + lx] : 0.f;
    }
    return raw ? raw_px(rs, H, W, gx, gy) : px(src, H, W, gx, gy);
  };
  f32x4 cq = {0.f, 0.f, 0.f, 0.f};
  if (raw && mode == MDS_AUG_COPY) cq = raw_quad(rs, W, x0, y);      // COPY of a raw source: the plain pad + normalize
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + j;
    float r = 0.0f;
    if (x < W) {
      if (mode == MDS_AUG_COPY) {
        r = raw ? cq[j] : src[(long)y * W + x];
      } else if (mode == MDS_AUG_WARP) {
        // torch grid_sample(bilinear, zeros, align_corners=True): pixel coordinates, each corner weighted if inside
        const float sx = m[0] * (float)x + m[1] * (float)y + m[2], sy = m[3] * (float)x + m[4] * (float)y + m[5];
        const float fx = floorf(sx), fy = floorf(sy);
        const float wx1 = sx - fx, wy1 = sy - fy, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
        // (far outside the frame every corner is masked; the select only keeps the float -> int conversions defined)
        const bool near = sx > -2.0f && sx < (float)W + 1.0f && sy > -2.0f && sy < (float)H + 1.0f;
        const int jx = near ? (int)fx : -2, jy = near ? (int)fy : -2;
        r = tap(jx, jy) * (wx0 * wy0) + tap(jx + 1, jy) * (wx1 * wy0) + tap(jx, jy + 1) * (wx0 * wy1) + tap(jx + 1, jy + 1) * (wx1 * wy1);
      } else if (mode == MDS_AUG_SHARP) {
        const float c = tap(x, y);
        if (x >= 1 && x < W - 1 && y >= 1 && y < H - 1) {
          float s_ = tap(x - 1, y - 1) + tap(x, y - 1) + tap(x + 1, y - 1) + tap(x - 1, y) + 5.0f * c + tap(x + 1, y) +
                     tap(x - 1, y + 1) + tap(x, y + 1) + tap(x + 1, y + 1);
          s_ = fminf(fmaxf(s_ * (1.0f / 13.0f), 0.0f), 1.0f);
          r = s_ + (c - s_) * jb.sharp_factor;         // factor in (0, 1): no clamp (kornia _blend_one)
        } else {
          r = c;                                       // border pixels keep their value
        }
      } else if (staged) {   // MDS_AUG_TAPS from the staged box: every tap of every pixel of the tile lies inside it (checked above)
        const float* c0 = tile + (y - by0) * bw + (x - bx0);
        for (int k = 0; k < ntaps; ++k) r += tapw[k] * c0[tapo[k]];
      } else {
        for (int k = 0; k < jb.ntaps; ++k) r += jb.tap_w[k] * tap(x + jb.tap_dx[k], y + jb.tap_dy[k]);
      }
    }
    v[j] = r;
  }
  if (jb.point) {
    if (jb.bright_on) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fminf(fmaxf(v[j] + jb.bright_add, 0.0f), 1.0f);
    }
    if (jb.contrast_on) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fminf(fmaxf(v[j] * jb.contrast_mul, 0.0f), 1.0f);
    }
    if (jb.posterize_bits > 0) {
      const int sh = 8 - jb.posterize_bits;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned u = (unsigned)(unsigned char)(int)(v[j] * 255.0f);     // torch .to(uint8): truncation
        v[j] = (float)((u >> sh) << sh) / 255.0f;
      }
    }
    if (jb.noise_on) {
      float z[4];
      if (a.noise) {
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = (x0 + j < W) ? a.noise[plane_off + (long)y * W + x0 + j] : 0.0f;
      } else {     // counter = this quad's index in the (B, T, H, ceil(W / 4)) order: a function of (seed, element) only
        normal4((uint32_t)jb.noise_seed, (unsigned long long)((((long)b * a.T + t) * H + y) * (long)((W + 3) >> 2) + (x0 >> 2)), z);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = v[j] + z[j] * jb.noise_std + jb.noise_mean;
    }
  }
  float* o = dst + (long)y * W + x0;
  if (x0 + 3 < W && ((W & 3) == 0)) {
    *(f32x4*)o = (f32x4){v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < W) o[j] = v[j];
  }
}

extern "C" int mds_aug_pass(const mds_aug_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a && a->B > 0 && a->T > 0 && a->H > 0 && a->W > 0 && a->jobs && (a->buf[0] || a->raw.u8) && a->buf[1], "aug_pass: bad args");
  MDS_REQUIRE((long)a->H * a->W < 2147483647L, "aug_pass: frame too large");
  if (a->raw.u8) {
    const mds_aug_raw_t& r = a->raw;
    MDS_REQUIRE(r.src_h >= 1 && r.src_w >= 1 && r.pad_top >= 0 && r.pad_left >= 0 && (long)r.pad_top + r.src_h <= a->H && (long)r.pad_left + r.src_w <= a->W,
                "aug_pass: raw source %d x %d at (%d, %d) of a %d x %d frame", r.src_h, r.src_w, r.pad_top, r.pad_left, a->H, a->W);
    MDS_REQUIRE(r.fill >= 0 && r.fill <= 255, "aug_pass: raw fill = %d (a byte value)", r.fill);
  }
  const int bx = cdiv(a->H, AUG_TR) * cdiv(a->W, AUG_TC);      // one block per 8 x 128 output tile
  MDS_REQUIRE(a->T <= 65535 && a->B <= 65535, "aug_pass: grid");
  MDS_LAUNCH(aug_kernel, dim3(bx, a->T, a->B), dim3(256), 0, stream, *a);
  return mds_check_launch("aug_pass");
}

// ------------------------------------------------------------------ the frames processor alone: uint8 planes -> padded fp32 planes
// HBM streaming: 1 byte read and 4 bytes written per output pixel.  One work item = four consecutive columns of one output row:
// one 4-byte load (raw_quad) and one 16-byte store per lane, a wave covers 256 contiguous source bytes and 1 KiB of output.
// grid = (pieces of a plane's H * ceil(W / 4) items, planes), both grid-strided.
__global__ __launch_bounds__(256) void pad_normalize_kernel(mds_pad_normalize_args a) {
  const int H = a.H, W = a.W;
  const unsigned nq = ((unsigned)W + 3u) >> 2, items = (unsigned)H * nq;      // < 2^31: H * W is
  const float fillv = u8_unit((unsigned)a.fill);
  const bool vec = (W & 3) == 0 && ((uintptr_t)a.dst & 15) == 0;      // then every row of every plane starts 16-byte aligned
  for (long n = blockIdx.y; n < a.n; n += gridDim.y) {
    const RawPlane rs = {a.src + n * a.src_h * a.src_w, a.src_h, a.src_w, a.pad_top, a.pad_left, fillv};
    float* plane = a.dst + n * H * W;
    for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
      const unsigned y = it / nq;
      const int x0 = (int)((it - y * nq) << 2);
      const f32x4 v = raw_quad(rs, W, x0, (int)y);
      float* o = plane + (long)y * W + x0;
      if (vec) *(f32x4*)o = v;
      else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < W) o[j] = v[j];
      }
    }
  }
}
extern "C" long mds_pad_normalize(const mds_pad_normalize_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a && a->src && a->dst, "pad_normalize: null pointer");
  MDS_REQUIRE(a->n >= 1 && a->H > 0 && a->W > 0 && (long)a->H * a->W < 2147483647L, "pad_normalize: n = %ld planes of %d x %d", a->n, a->H, a->W);
  MDS_REQUIRE(a->src_h >= 1 && a->src_w >= 1 && a->pad_top >= 0 && a->pad_left >= 0 && (long)a->pad_top + a->src_h <= a->H && (long)a->pad_left + a->src_w <= a->W,
              "pad_normalize: source %d x %d at (%d, %d) of a %d x %d frame", a->src_h, a->src_w, a->pad_top, a->pad_left, a->H, a->W);
  MDS_REQUIRE(a->fill >= 0 && a->fill <= 255, "pad_normalize: fill = %d (a byte value)", a->fill);
  const long cap = mds_knob(MDS_KNOB_STREAM_BLOCKS) ? mds_knob(MDS_KNOB_STREAM_BLOCKS) : 2048;      // as elem.h::stream_blocks
  const long items = (long)a->H * ((a->W + 3) / 4);
  long by = a->n < cap ? a->n : cap;
  by = by > 65535 ? 65535 : by;
  long bx = (items + 255) / 256, per = (cap + by - 1) / by;      // about `cap` blocks in all
  bx = bx > per ? per : bx;
  MDS_LAUNCH(pad_normalize_kernel, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, stream, *a);
  return mds_check_launch("pad_normalize");
}

// ------------------------------------------------------------------ SURVEY 8(f) N4, device side: pitched luma plane -> frames
// HBM streaming copy: 16 bytes per lane where source row and destination row are both 16-byte aligned, bytes otherwise.
__global__ __launch_bounds__(256) void frame_luma_kernel(mds_frame_luma_args a) {
  const int f = blockIdx.z, y = blockIdx.y;
  const unsigned char* s = a.src + (long)f * a.surface_stride + (long)y * a.pitch;
  unsigned char* d = a.dst + ((long)f * a.height + y) * a.width;
  const bool vec = ((((uintptr_t)s) | ((uintptr_t)d)) & 15) == 0;
  const int nv = vec ? a.width >> 4 : 0;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < nv; v += gridDim.x * 256) ((u32x4*)d)[v] = ((const u32x4*)s)[v];
  for (int x = 16 * nv + blockIdx.x * 256 + threadIdx.x; x < a.width; x += gridDim.x * 256) d[x] = s[x];
}
extern "C" int mds_frame_luma(const mds_frame_luma_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a && a->src && a->dst && a->width > 0 && a->height > 0 && a->count > 0, "frame_luma: bad args");
  MDS_REQUIRE(a->pitch >= a->width && a->height <= 65535 && a->count <= 65535, "frame_luma: pitch must cover a row; at most 65535 rows / surfaces");
  MDS_LAUNCH(frame_luma_kernel, dim3(cdiv(a->width, 16 * 256) > 0 ? cdiv(a->width, 16 * 256) : 1, a->height, a->count), dim3(256), 0, stream, *a);
  return mds_check_launch("frame_luma");
}

// ------------------------------------------------------------------ predictor glue, slot-addressed row copies
// One launch moves the rows a predictor step needs between its device rings and a plan's buffers; the slot numbers are kernel
// arguments (an index tensor would be a host-to-device copy per frame).  grid = (pieces of a row, rows).
__global__ __launch_bounds__(256) void copy_rows_kernel(mds_copy_rows_args a) {
  const int r = blockIdx.y;
  const unsigned char* s = (const unsigned char*)a.src + (long)a.src_slot[r] * a.src_pitch;
  unsigned char* d = (unsigned char*)a.dst + (long)a.dst_slot[r] * a.dst_pitch;
  const bool vec = ((((uintptr_t)s) | ((uintptr_t)d)) & 15) == 0;
  const long nv = vec ? a.row_bytes >> 4 : 0;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long)gridDim.x * 256) ((u32x4*)d)[v] = ((const u32x4*)s)[v];
  for (long x = 16 * nv + (long)blockIdx.x * 256 + threadIdx.x; x < a.row_bytes; x += (long)gridDim.x * 256) d[x] = s[x];
}
extern "C" int mds_copy_rows(const mds_copy_rows_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a && a->src && a->dst && a->row_bytes > 0 && a->nrows > 0 && a->nrows <= MDS_COPY_ROWS_MAX, "copy_rows: bad args (at most %d rows)", MDS_COPY_ROWS_MAX);
  for (int r = 0; r < a->nrows; ++r) MDS_REQUIRE(a->dst_slot[r] >= 0 && a->src_slot[r] >= 0, "copy_rows: negative slot");
  long bx = cdiv(a->row_bytes, 16L * 256 * 4);      // four 16-byte vectors per lane
  bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
  MDS_LAUNCH(copy_rows_kernel, dim3((unsigned)bx, a->nrows), dim3(256), 0, stream, *a);
  return mds_check_launch("copy_rows");
}
