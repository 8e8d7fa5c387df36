// k_dwx.hip — the 2D depthwise forward with the block's 1x1 expansion as its prologue (inference plans, mds_expand_t).
//
// An inverted-residual block's expanded tensor y1 = silu(bn1(x * w^T)) only feeds the depthwise conv that follows it.
// Here a block owns a tile of output pixels and DWX_MC mid channels:
//   1. the input halo tile of x (cin wide) is staged in LDS DWX_KC channels at a time (the next chunk's global loads are
//      in flight while the current one is multiplied);
//   2. y1 for the halo tile is an MFMA GEMM [halo pixels x cin] * [cin x DWX_MC], accumulated in registers, activated
//      (BN1 + SiLU) and written to LDS as fp32 - zero where the halo leaves the image (padding of the ACTIVATED tensor);
//   3. the 3x3 depthwise, the output transform (BN2 + SiLU), the store and the squeeze-excite pool read y1 from LDS.
// Tiles: stride 1 = 8 x 8 outputs (10 x 10 halo, 1.56x recomputation), stride 2 = 4 x 8 outputs (9 x 17 halo, 1.2x).
// LDS: the x chunks and the y1 tile share one buffer (the GEMM is done before y1 is written): 27 KiB (stride 1) /
// 41 KiB (stride 2), i.e. 5 / 3 blocks per CU by LDS.  fp32 x is split into hi / lo bf16 halves while it is staged
// (split-bf16 product, Mma<float, true>: the numerics of the inference pw_fwd); bf16 runs one MFMA per fragment pair.
#include "gemm.h"
#include "se_tail.h"

#define DWX_MC 64   // mid channels per block (4 waves x one 16-column MFMA tile)
#define DWX_KC 32   // input channels per staged chunk (one MFMA k step)
#define DWX_SE_RH 2 // rows of w1 in flight per wave in the squeeze-excite tail (se_tail.h): stays under the kernel's own ~100 VGPRs

template <int S> struct DwxTile;
template <> struct DwxTile<1> { static const int TOH = 8, TOW = 8; };
template <> struct DwxTile<2> { static const int TOH = 4, TOW = 8; };

template <typename T, int S> struct DwxGeo {
  static const int TOH = DwxTile<S>::TOH, TOW = DwxTile<S>::TOW;
  static const int HH = (TOH - 1) * S + 3, HW = (TOW - 1) * S + 3;   // halo tile
  static const int P = HH * HW, MT = (P + 15) / 16, PP = MT * 16;    // halo pixels, MFMA row tiles
  static const int XP = DWX_KC + 8;                                  // bf16 pitch of a staged row (16-byte aligned, skewed banks)
  static const int NX = sizeof(T) == 4 ? 2 : 1;                      // staged halves: hi / lo (fp32) or the value (bf16)
  static const int YP = DWX_MC + 4;                                  // fp32 pitch of the y1 tile
  static const int NU = (PP * (DWX_KC / 8) + 255) / 256;             // 8-channel staging units per thread
  static const int XBYTES = NX * PP * XP * 2, YBYTES = P * YP * 4;
  static const int SMEM = XBYTES > YBYTES ? XBYTES : YBYTES;
};

// A operand staged in LDS / B operand read from the packed filter, per storage type
template <typename T> struct DwxOp;
template <> struct DwxOp<bf16_t> {
  typedef u16x8 frag;
  static MDS_DEV void stage(bf16_t* hi, bf16_t*, const RawV8<bf16_t>& r) { *(u16x8*)hi = r.v; }
  static MDS_DEV frag a(const bf16_t* hi, const bf16_t*) { return *(const u16x8*)hi; }
  static MDS_DEV frag b(const bf16_t* w, bool ok) {
    u16x8 v = (u16x8){0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) v = *(const u16x8*)w;
    return v;
  }
};
template <> struct DwxOp<float> {
  typedef FragX3 frag;
  static MDS_DEV void stage(bf16_t* hi, bf16_t* lo, const RawV8<float>& r) {
    const FragX3 f = split_x3((f32x8){r.a[0], r.a[1], r.a[2], r.a[3], r.b[0], r.b[1], r.b[2], r.b[3]});
    *(u16x8*)hi = f.hi;
    *(u16x8*)lo = f.lo;
  }
  static MDS_DEV frag a(const bf16_t* hi, const bf16_t* lo) {
    FragX3 f;
    f.hi = *(const u16x8*)hi;
    f.lo = *(const u16x8*)lo;
    return f;
  }
  static MDS_DEV frag b(const float* w, bool ok) {
    f32x8 v = (f32x8){0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) v = ld_frag(w);
    return split_x3(v);
  }
};

template <typename T, int S, int POOL>   // POOL = 1: squeeze-excite pool, 2: pool + the squeeze-excite tail (mds_se_tail_t)
__global__ __launch_bounds__(256) void dwx_fwd_kernel(mds_dw_fwd_args a, int tiles_x, int tiles_y, int nchunks) {
  MDS_CHAIN_PRIO();
  typedef DwxGeo<T, S> G;
  typedef Mma<T, sizeof(T) == 4> MM;
  MDS_DYN_SMEM(smem);
  bf16_t* xs = (bf16_t*)smem;   // [NX][PP][XP] staged x chunk
  float* ys = (float*)smem;     // [P][YP] y1 tile (after the GEMM; same memory)
  __shared__ float red[4][DWX_MC];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  // work sequence: channel chunk fastest, so the blocks that re-read one halo tile of x run next to each other on one XCD
  const unsigned s = xcd_contiguous(blockIdx.x, gridDim.x);
  const int chunk = (int)(s % (unsigned)nchunks);
  int t = (int)(s / (unsigned)nchunks);
  const int tx = t % tiles_x;
  t /= tiles_x;
  const int ty = t % tiles_y, n = t / tiles_y;
  const int oy0 = ty * G::TOH, ox0 = tx * G::TOW, iy0 = oy0 * S - a.pad_t, ix0 = ox0 * S - a.pad_l;
  const int C = a.C, cin = a.expand.cin, c0 = chunk * DWX_MC, IH = a.IH, IW = a.IW;
  const T* xim = (const T*)a.expand.x + (long)n * IH * IW * cin;

  // ---- 1 + 2: y1[halo pixel][16 channels of this wave] = x * w^T, K-chunked through LDS
  const int cw = c0 + 16 * wave + li;   // B column of this lane (C % 16 == 0: a wave's 16 columns are all valid or all not)
  const bool cwok = cw < C;
  const T* wrow = (const T*)a.expand.w + (long)(cwok ? cw : 0) * cin;
  f32x4 acc[G::MT];
#pragma unroll
  for (int m = 0; m < G::MT; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
  RawV8<T> raw[G::NU];
  auto load = [&](int k0) {
#pragma unroll
    for (int j = 0; j < G::NU; ++j) {
      const int u = tid + 256 * j, p = u >> 2, k = k0 + (u & 3) * 8;
      const int hy = p / G::HW, hx = p - hy * G::HW, iy = iy0 + hy, ix = ix0 + hx;
      if (p < G::P && k < cin && iy >= 0 && iy < IH && ix >= 0 && ix < IW) raw[j].ld(xim + ((long)iy * IW + ix) * cin + k);
      else raw[j].zero();
    }
  };
  load(0);
  for (int k0 = 0; k0 < cin; k0 += DWX_KC) {
#pragma unroll
    for (int j = 0; j < G::NU; ++j) {
      const int u = tid + 256 * j, p = u >> 2, ko = (u & 3) * 8;
      if (p < G::PP) DwxOp<T>::stage(xs + p * G::XP + ko, xs + (G::PP + p) * G::XP + ko, raw[j]);
    }
    const typename DwxOp<T>::frag b = DwxOp<T>::b(wrow + k0 + 8 * lq, cwok && k0 + 8 * lq < cin);
    __syncthreads();
    if (k0 + DWX_KC < cin) load(k0 + DWX_KC);   // next chunk in flight during the products
#pragma unroll
    for (int m = 0; m < G::MT; ++m) {
      const int r = (m * 16 + li) * G::XP + 8 * lq;
      MM::mma(DwxOp<T>::a(xs + r, xs + G::PP * G::XP + r), b, acc[m]);
    }
    __syncthreads();
  }
  // activation into the y1 tile: C[row 4q + r][col i] of row tile m is halo pixel 16m + 4q + r, channel 16 * wave + i
  {
    const float s1 = cwok ? a.expand.scale[cw] : 0.f, b1 = cwok ? a.expand.shift[cw] : 0.f;
#pragma unroll
    for (int m = 0; m < G::MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = m * 16 + 4 * lq + r;
        if (p >= G::P) continue;
        const int hy = p / G::HW, hx = p - hy * G::HW, iy = iy0 + hy, ix = ix0 + hx;
        const bool in = iy >= 0 && iy < IH && ix >= 0 && ix < IW;
        ys[p * G::YP + 16 * wave + li] = in ? siluf_(acc[m][r] * s1 + b1) : 0.f;   // zero padding AFTER the activation
      }
  }
  __syncthreads();

  // ---- 3: depthwise 3x3 + output transform + pool; a thread = 4 channels x every 16th output pixel of the tile
  const int cg = tid & 15, pg = tid >> 4, c = c0 + 4 * cg;
  const bool cok = c < C;
  float wd[9][4], esc[4], esh[4], psum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int k = 0; k < 9; ++k) wd[k][j] = cok ? a.w[(long)(c + j) * 9 + k] : 0.f;
    esc[j] = cok ? a.epi.scale[c + j] : 0.f;
    esh[j] = cok ? a.epi.shift[c + j] : 0.f;
  }
  const int emode = a.epi.mode;
  T* yim = (T*)a.y + (long)n * a.OH * a.OW * C + c;
#pragma unroll
  for (int j = 0; j < G::TOH * G::TOW / 16; ++j) {
    const int o = pg + 16 * j, ry = o / G::TOW, rx = o - ry * G::TOW, oy = oy0 + ry, ox = ox0 + rx;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const f32x4 yv = *(const f32x4*)(ys + ((ry * S + ky) * G::HW + rx * S + kx) * G::YP + 4 * cg);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] += yv[q] * wd[ky * 3 + kx][q];
      }
    if (cok && oy < a.OH && ox < a.OW) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = v[q] * esc[q] + esh[q];
        if (emode == MDS_EPI_BN_SILU) v[q] = siluf_(v[q]);
        if (POOL) psum[q] += Elem<T>::rnd(v[q]);   // the means of the STORED output
      }
      store4(yim + ((long)oy * a.OW + ox) * C, v);
    }
  }
  if (POOL) {
    // the four pixel groups of a wave that share a channel group: lanes cg, cg + 16, cg + 32, cg + 48
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      psum[q] += __shfl_xor(psum[q], 16);
      psum[q] += __shfl_xor(psum[q], 32);
    }
    if (lane < 16) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[wave][4 * cg + q] = psum[q];
    }
    __syncthreads();
    if (tid < DWX_MC && c0 + tid < C) {
      const float tot = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
      atomicAdd(a.pool + (long)n * C + c0 + tid, (double)(tot * a.pool_inv));
    }
    if (POOL == 2) {   // a block is one (tile, channel chunk) of image n: one ticket each
      __shared__ int se_img[8];
      if (tid < 8) se_img[tid] = tid == 0 ? n : -1;
      se_tail_tickets<DWX_SE_RH>(a.se, a.pool, C, se_img, tiles_x * tiles_y * nchunks);
    }
  }
}

template <typename T, int S>
static void dwx_launch(const mds_dw_fwd_args* a, mds_stream_t stream) {
  typedef DwxGeo<T, S> G;
  const int tiles_x = cdiv(a->OW, G::TOW), tiles_y = cdiv(a->OH, G::TOH), nchunks = cdiv(a->C, DWX_MC);
  const dim3 grid((unsigned)((long)a->N * tiles_y * tiles_x * nchunks)), block(256);
  if (a->se.gate) MDS_LAUNCH((dwx_fwd_kernel<T, S, 2>), grid, block, G::SMEM, stream, *a, tiles_x, tiles_y, nchunks);
  else if (a->pool) MDS_LAUNCH((dwx_fwd_kernel<T, S, 1>), grid, block, G::SMEM, stream, *a, tiles_x, tiles_y, nchunks);
  else MDS_LAUNCH((dwx_fwd_kernel<T, S, 0>), grid, block, G::SMEM, stream, *a, tiles_x, tiles_y, nchunks);
}

// mds_dw_fwd with a->expand.x set (k_dw.hip routes here)
int dw_fwd_expand(const mds_dw_fwd_args* a, mds_stream_t stream) {
  const mds_expand_t& e = a->expand;
  MDS_REQUIRE(a->N > 0 && a->T == 1 && a->kt == 1 && a->IH > 0 && a->IW > 0, "dw_fwd (expand): 2D only (T == 1, kt == 1)");
  MDS_REQUIRE(a->stride == 1 || a->stride == 2, "dw_fwd (expand): stride");
  MDS_REQUIRE(a->C > 0 && a->C % 16 == 0 && e.cin > 0 && e.cin % 8 == 0, "dw_fwd (expand): needs C %% 16 == 0 and cin %% 8 == 0");
  MDS_REQUIRE(e.w && e.scale && e.shift && a->w && a->y, "dw_fwd (expand): null pointer");
  MDS_REQUIRE(a->pro.mode == MDS_PRO_NONE && !a->stats, "dw_fwd (expand): no prologue, no statistics");
  MDS_REQUIRE((a->epi.mode == MDS_EPI_AFFINE || a->epi.mode == MDS_EPI_BN_SILU) && a->epi.scale && a->epi.shift,
              "dw_fwd (expand): needs an output transform");
  if (a->se.gate) SE_TAIL_REQUIRE(a, "dw_fwd (expand)");
  MDS_REQUIRE(!a->pool || a->pool_inv > 0.f, "dw_fwd (expand): pool_inv");
  if (a->stride == 1) {
    MDS_REQUIRE(a->pad_t == 1 && a->pad_l == 1 && a->OH == a->IH && a->OW == a->IW, "dw_fwd (expand): stride-1 geometry");
  } else {
    MDS_REQUIRE(a->pad_t >= 0 && a->pad_t <= 1 && a->pad_l >= 0 && a->pad_l <= 1 && a->OH == (a->IH + 1) / 2 && a->OW == (a->IW + 1) / 2,
                "dw_fwd (expand): stride-2 geometry");
  }
  MDS_REQUIRE((long)a->N * cdiv(a->OH, 4) * cdiv(a->OW, 8) * cdiv(a->C, DWX_MC) < 2147483647L, "dw_fwd (expand): grid");
  if (a->stride == 1) MDS_DISPATCH_DTYPE(a->dtype, T, (dwx_launch<T, 1>(a, stream)));
  else MDS_DISPATCH_DTYPE(a->dtype, T, (dwx_launch<T, 2>(a, stream)));
  return mds_check_launch("dw_fwd (expand)");
}
