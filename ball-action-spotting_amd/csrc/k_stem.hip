// k_stem.hip — the stem: 3x3 stride-2 TF-SAME convolution of the fp32 frame triple.
//
// Input is the (b*S, 3, H, W) fp32 view of the frame stack (multidim_stacker.py:214): three
// grayscale planes per image.  K = 27 (padded to 32) is a single MFMA k-step, so the kernel is a
// pure streaming pass: 226 MB of frames in, 301 MB of bf16 activations out per batch-4 step
// (15 FLOP/B -> HBM-bound).  im2col fragments are gathered straight from global memory (the
// planes are read with unit stride along W by neighbouring lanes), weights live in registers.
#include <stdlib.h>
#include "gemm.h"

template <typename T>
__global__ __launch_bounds__(256) void stem_fwd_kernel(mds_stem_fwd_args a) {
  MDS_CHAIN_PRIO();
  typedef typename Frag<T>::type frag_t;
  const int tid = threadIdx.x, lane = tid & 63;
  const int i = lane & 15, q = lane >> 4;
  // XCD-aware: consecutive block ids go to consecutive XCDs, each with its own L2.  A wave's 16-pixel group reads 33 input
  // columns of 3 rows: the boundary line of a block's four groups and two of the three rows are shared with the neighbouring
  // blocks - on eight different XCDs each of them fetched the shared lines from HBM again (PMC round 4: 416 MB fetched for a
  // 226 MB input).  Every XCD now walks a contiguous range of the group sequence.
  const int gw = xcd_contiguous(blockIdx.x, gridDim.x) * 4 + (tid >> 6), nw = gridDim.x * 4;
  const T* w = (const T*)a.w;
  frag_t wf[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    if (16 * f + i < a.Cout) wf[f] = ld_frag(w + (16 * f + i) * 32 + 8 * q);
    else frag_zero(wf[f]);
  }
  int tp[8], tky[8], tkx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * q + j;
    tp[j] = k < 27 ? k / 9 : -1;
    tky[j] = (k % 9) / 3;
    tkx[j] = k % 3;
  }
  const int gpr = (a.OW + 15) / 16;  // 16-pixel groups per output row
  const long ngroups = (long)a.N * a.OH * gpr;
  float s_[8], ss_[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s_[e] = 0.f; ss_[e] = 0.f; }
  T* y = (T*)a.y;
  const int emode = a.epi.mode;       // eval-mode output transform (mds_epi_t): this lane's 2 x 4 output channels
  float es[2][4], eh[2][4];
  if (emode != MDS_EPI_NONE) {
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int oc = 16 * f + 4 * q + rr;
        es[f][rr] = oc < a.Cout ? a.epi.scale[oc] : 0.f;
        eh[f][rr] = oc < a.Cout ? a.epi.shift[oc] : 0.f;
      }
  }
  for (long gi = gw; gi < ngroups; gi += nw) {
    const int gx = (int)(gi % gpr);
    long r = gi / gpr;
    const int oy = (int)(r % a.OH);
    const int n = (int)(r / a.OH);
    const int ox = gx * 16 + i;
    frag_t xf;
    float xv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int iy = oy * 2 + tky[j] - a.pad_t, ix = ox * 2 + tkx[j] - a.pad_l;
      xv[j] = 0.f;
      if (tp[j] >= 0 && ox < a.OW && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
        if (a.ingest.u8) {   // raw uint8 frame: pad + /255 (+ mirrored re-read for the TTA copies) while gathering
          const int ns = n < a.ingest.nsrc ? n : n - a.ingest.nsrc;
          const int sy = iy - a.ingest.pad_top, sx = (n < a.ingest.nsrc ? ix : a.W - 1 - ix) - a.ingest.pad_left;
          if (sy >= 0 && sy < a.ingest.src_h && sx >= 0 && sx < a.ingest.src_w)
            xv[j] = (float)a.ingest.u8[(((long)ns * 3 + tp[j]) * a.ingest.src_h + sy) * a.ingest.src_w + sx] * a.ingest.scale;
        } else {
          xv[j] = a.x[(((long)n * 3 + tp[j]) * a.H + iy) * a.W + ix];
        }
      }
    }
    frag_from8(xf, xv);
    f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
    mma16(wf[0], xf, acc[0]);  // acc[r] = y[pixel i][oc = 4q + r]
    mma16(wf[1], xf, acc[1]);
    if (ox < a.OW) {
      const long row = ((long)n * a.OH + oy) * a.OW + ox;
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const int oc = 16 * f + 4 * q;
        if (oc < a.Cout) {
          float v[4] = {acc[f][0], acc[f][1], acc[f][2], acc[f][3]};
          if (emode != MDS_EPI_NONE) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              const float z = v[rr] * es[f][rr] + eh[f][rr];
              v[rr] = emode == MDS_EPI_BN_SILU ? siluf_(z) : z;
            }
          }
          store4(y + row * a.Cout + oc, v);
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) { s_[f * 4 + rr] += v[rr]; ss_[f * 4 + rr] += v[rr] * v[rr]; }
        }
      }
    }
  }
  if (a.stats) {
    double* st = a.stats + (long)(blockIdx.x % MDS_STAT_SLOTS) * 2 * a.Cout;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float s = sum_over_i16(s_[e]), ss = sum_over_i16(ss_[e]);
      const int oc = 16 * (e >> 2) + 4 * q + (e & 3);
      if (i == 0 && oc < a.Cout) { atomicAdd(st + oc, (double)s); atomicAdd(st + a.Cout + oc, (double)ss); }
    }
  }
}

static int stem_fwd_tiled(const mds_stem_fwd_args* a, mds_stream_t stream);
extern "C" int mds_stem_fwd(const mds_stem_fwd_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a && a->N > 0 && a->H > 0 && a->W > 0 && a->OH > 0 && a->OW > 0, "stem_fwd: bad dims");
  MDS_REQUIRE(a->Cout % 16 == 0 && a->Cout <= 32, "stem_fwd: Cout=%d must be 16 or 32", a->Cout);
  MDS_REQUIRE((a->x || a->ingest.u8) && a->w && a->y, "stem_fwd: null pointer");
  MDS_REQUIRE(!a->ingest.u8 || (a->ingest.nsrc > 0 && a->ingest.src_h > 0 && a->ingest.src_w > 0 && a->N <= 2 * a->ingest.nsrc),
              "stem_fwd: ingest needs nsrc, src_h, src_w and N <= 2 * nsrc");
  if (a->dtype == MDS_BF16 && a->x && !a->ingest.u8 && a->epi.mode == MDS_EPI_NONE && mds_knob(MDS_KNOB_STEM_FWD) != 1)
    return stem_fwd_tiled(a, stream);                  // the training forward (k_stem.hip, below)
  const long ngroups = (long)a->N * a->OH * ((a->OW + 15) / 16);
  long nb = (ngroups + 3) / 4;
  if (nb > 4096) nb = 4096;
  MDS_DISPATCH_DTYPE(a->dtype, T, MDS_LAUNCH(stem_fwd_kernel<T>, dim3((unsigned)nb), dim3(256), 0, stream, *a));
  return mds_check_launch("stem_fwd");
}

// weight gradient: dw[oc][27] += sum_pixels dy[pixel][oc] * x27[pixel][k]; the MFMA reduction
// index runs over 32 consecutive output pixels of one row.
template <typename T>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(mds_stem_wgrad_args a) {
  typedef typename Frag<T>::type frag_t;
  const int tid = threadIdx.x, lane = tid & 63;
  const int i = lane & 15, q = lane >> 4;
  const int gw = blockIdx.x * 4 + (tid >> 6), nw = gridDim.x * 4;
  const T* dy = (const T*)a.dy;
  int tp[2], tky[2], tkx[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int k = 16 * g + i;
    tp[g] = k < 27 ? k / 9 : -1;
    tky[g] = (k % 9) / 3;
    tkx[g] = k % 3;
  }
  const int gpr = (a.OW + 31) / 32;
  const long ngroups = (long)a.N * a.OH * gpr;
  f32x4 acc[2][2];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int g = 0; g < 2; ++g) acc[f][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const bool det = a.partial.buf != nullptr;      // deterministic way out: every WAVE holds a whole filter gradient - slot = global wave index
  float* const dw = wg_base(a.dw, a.partial, (long)a.Cout * 27, gw);
  for (long gi = gw; gi < ngroups; gi += nw) {
    const int gx = (int)(gi % gpr);
    long r = gi / gpr;
    const int oy = (int)(r % a.OH);
    const int n = (int)(r / a.OH);
    const int oxb = gx * 32 + 8 * q;  // this lane's 8 pixels
    const long rowb = ((long)n * a.OH + oy) * a.OW;
    frag_t yf[2], xf[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      float yv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ox = oxb + j, oc = 16 * f + i;
        yv[j] = (ox < a.OW && oc < a.Cout) ? Elem<T>::ld(dy + (rowb + ox) * a.Cout + oc) : 0.f;
      }
      frag_from8(yf[f], yv);
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int iy = oy * 2 + tky[g] - a.pad_t;
      float xv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ox = oxb + j, ix = ox * 2 + tkx[g] - a.pad_l;
        xv[j] = 0.f;
        if (tp[g] >= 0 && ox < a.OW && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
          xv[j] = a.x[(((long)n * 3 + tp[g]) * a.H + iy) * a.W + ix];
      }
      frag_from8(xf[g], xv);
    }
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int g = 0; g < 2; ++g) mma16(yf[f], xf[g], acc[f][g]);  // acc[r] = dw[oc = 4q + r][k = i]
  }
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int k = 16 * g + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oc = 16 * f + 4 * q + r;
        if (k < 27 && oc < a.Cout) wg_out(dw + oc * 27 + k, acc[f][g][r], det);
      }
    }
}

// bf16 variant, tiled through LDS (the gather kernel above issues 32 scalar loads per MFMA group and
// runs at 0.9 TB/s).  Tile = 8 output rows x 32 output columns; per (plane, input row) three arrays
// A_kx[j] = x[2(ox0+j) + kx - pad_l] are staged (9 coalesced 8-byte loads -> three 16-byte LDS
// stores per item), so a tap's fragment — 8 consecutive output columns of one (plane, ky, kx) — is ONE
// aligned 16-byte LDS read; dy is staged as loaded ([pixel][oc]) and read with the transposing
// ds_read_b64_tr_b16.  Persistent blocks, next tile's loads in flight under the MFMAs.
#define SW_ROWS 8
#define SW_COLS 32
#define SW_PITCH 48   // elements: 96 B = 32 B x odd (conflict-free for ds_read_b128 and the tr reads)
template <bool DYP>
__global__ __launch_bounds__(256, DYP ? 2 : 3) void stem_wgrad_tiled_kernel(mds_stem_wgrad_args a, int tiles_a, int tiles_b, int tiles_per_block) {
  typedef bf16_t T;
  constexpr int IR = 2 * SW_ROWS + 1;                  // input rows of a tile
  constexpr int NX = IR * 3 * (SW_COLS / 8);           // x staging items: (input row, plane, 8-column group)
  MDS_DYN_SMEM(smem);
  T* xa = (T*)smem;                                    // [IR][3 planes][3 kx][SW_PITCH]
  T* dys = xa + IR * 9 * SW_PITCH;                     // [SW_ROWS * SW_COLS][SW_PITCH]
  T* zrow = dys + SW_ROWS * SW_COLS * SW_PITCH;        // [SW_PITCH] zeros (k = 27..31)
  const int tid = threadIdx.x, lane = tid & 63, wave = MDS_UNIFORM(tid >> 6);
  const int i = lane & 15, q = lane >> 4;
  const T* dy = (const T*)(DYP ? a.dyp.g.u : a.dy);
  const long ydiff = DYP ? (const T*)a.dyp.y - dy : 0;   // the BatchNorm input y has u's layout
  // dy = A*g + B*y + D, g = u or u*silu'(y*scale + shift): this thread stages the same 8 channels of every pixel
  float cA[8], cB[8], cD[8], csc[8], csh[8];
  if (DYP) {
    const int c = 8 * (tid & 3), C = a.Cout;
    if (c < C) {
      load8f(a.dyp.lin + c, cA); load8f(a.dyp.lin + C + c, cB); load8f(a.dyp.lin + 2 * C + c, cD);
      load8f(a.dyp.bn + c, csc); load8f(a.dyp.bn + C + c, csh);
    }
  }
  const bool gsilu = DYP && a.dyp.g.mode == MDS_G_SILU;
  if (tid < SW_PITCH) zrow[tid] = 0;
  // this lane's two taps n = 16g + i -> (plane, ky, kx): LDS element offset of its row within the tile image
  int noff[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int n = 16 * g + i;
    const int pl = n / 9, ky = (n % 9) / 3, kx = n % 3;
    noff[g] = n < 27 ? ((ky * 3 + pl) * 3 + kx) * SW_PITCH : -1;   // + (2 r) * 9 * SW_PITCH per output row r
  }
  const long total = (long)a.N * tiles_a * tiles_b;
  long tl = (long)xcd_contiguous(blockIdx.x, gridDim.x) * tiles_per_block, tl_end = tl + tiles_per_block;
  if (tl_end > total) tl_end = total;
  f32x4 acc[2][2];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int g = 0; g < 2; ++g) acc[f][g] = (f32x4){0.f, 0.f, 0.f, 0.f};

  typedef float f32x2 __attribute__((ext_vector_type(2)));
  f32x2 rx[9];
  RawV8<T> ry[4], ryy[DYP ? 4 : 1];
  unsigned yok = 0;
  auto origin = [&](long t, int& img, int& oy0, int& ox0) {
    img = (int)(t / (tiles_a * tiles_b));
    const int rem = (int)(t - (long)img * tiles_a * tiles_b);
    oy0 = (rem / tiles_b) * SW_ROWS; ox0 = (rem % tiles_b) * SW_COLS;
  };
  auto issue = [&](long t) {
    int img, oy0, ox0;
    origin(t, img, oy0, ox0);
    if (tid < NX) {
      const int grp = tid & 3, pl = (tid >> 2) % 3, ir = tid / 12;
      const int iy = oy0 * 2 - a.pad_t + ir;
      const int iyc = iy < 0 ? 0 : (iy >= a.H ? a.H - 1 : iy);
      const float* row = a.x + (((long)img * 3 + pl) * a.H + iyc) * a.W;
      const int ix0 = 2 * (ox0 + 8 * grp) - a.pad_l;
      if (iy >= 0 && iy < a.H && ix0 >= 0 && ix0 + 17 < a.W) {   // interior: nine 8-byte loads
#pragma unroll
        for (int j = 0; j < 9; ++j) rx[j] = *(const f32x2*)(row + ix0 + 2 * j);
      } else {
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          const int ix = ix0 + 2 * j;
          const bool ok0 = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W, ok1 = iy >= 0 && iy < a.H && ix + 1 >= 0 && ix + 1 < a.W;
          const int c0 = ix < 0 ? 0 : (ix >= a.W ? a.W - 1 : ix), c1 = ix + 1 < 0 ? 0 : (ix + 1 >= a.W ? a.W - 1 : ix + 1);
          const float v0 = row[c0], v1 = row[c1];
          rx[j] = (f32x2){ok0 ? v0 : 0.f, ok1 ? v1 : 0.f};
        }
      }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int it = tid + 256 * p, px = it >> 2, ch = it & 3;
      const int oy = oy0 + (px >> 5), ox = ox0 + (px & 31);
      const bool ok = oy < a.OH && ox < a.OW && 8 * ch < a.Cout;
      if (ok) ry[p].ld(dy + (((long)img * a.OH + oy) * a.OW + ox) * a.Cout + 8 * ch);
      else ry[p].zero();
      if (DYP) {
        if (p == 0) yok = 0;
        yok |= (ok ? 1u : 0u) << p;
        if (ok) ryy[p].ld(dy + ydiff + (((long)img * a.OH + oy) * a.OW + ox) * a.Cout + 8 * ch);
        else ryy[p].zero();
      }
    }
  };
  if (tl < tl_end) issue(tl);
  for (; tl < tl_end; ++tl) {
    __syncthreads();
    if (tid < NX) {
      const int grp = tid & 3, pl = (tid >> 2) % 3, ir = tid / 12;
      T* base = xa + ((ir * 3 + pl) * 3) * SW_PITCH + 8 * grp;
      float v0[8], v1[8], v2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { v0[j] = rx[j][0]; v1[j] = rx[j][1]; v2[j] = rx[j + 1][0]; }
      store8(base, v0); store8(base + SW_PITCH, v1); store8(base + 2 * SW_PITCH, v2);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int it = tid + 256 * p;
      if (!DYP) {
        ry[p].st(dys + (it >> 2) * SW_PITCH + 8 * (it & 3));
      } else {
        float u[8], yv[8], v[8];
        ry[p].get(u);
        ryy[p].get(yv);
        const bool ok = (yok >> p) & 1u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float g = u[j];
          if (gsilu) g *= silu_gradf_(yv[j] * csc[j] + csh[j]);
          v[j] = ok ? cA[j] * g + cB[j] * yv[j] + cD[j] : 0.f;   // pixels past the image contribute nothing (D != 0)
        }
        store8(dys + (it >> 2) * SW_PITCH + 8 * (it & 3), v);
      }
    }
    __syncthreads();
    if (tl + 1 < tl_end) issue(tl + 1);
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int r = 2 * wave + rr;  // output row of the tile handled by this wave
      // A: dy^T fragments (8 pixels of one oc): pixels r*32 + 16(q>>1) + 4(q&1) + {0..3, 8..11}
      const int p0 = r * SW_COLS + 16 * (q >> 1) + 4 * (q & 1) + (i >> 2);
      u16x8 yf[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const T* pc = dys + 16 * f + 4 * (i & 3);
        const u16x4 lo = lds_tr4(pc + p0 * SW_PITCH), hi = lds_tr4(pc + (p0 + 8) * SW_PITCH);
        yf[f] = (u16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
      // B: x fragments: the same pixel permutation -> columns 16(q>>1) + 4(q&1) + {0..3} and +8
      const int cb = 16 * (q >> 1) + 4 * (q & 1);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const T* rowp = noff[g] >= 0 ? xa + (2 * r) * 9 * SW_PITCH + noff[g] : zrow;
        const int c = noff[g] >= 0 ? cb : 0;
        const u16x4 lo = *(const u16x4*)(rowp + c), hi = *(const u16x4*)(rowp + c + (noff[g] >= 0 ? 8 : 4));
        const u16x8 xf = (u16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int f = 0; f < 2; ++f) mma16(yf[f], xf, acc[f][g]);  // acc[r] = dw[oc = 16f + 4q + r][k = 16g + i]
      }
    }
  }
  // the 864 filter gradients are shared by every block: sum the four waves in LDS first, then one
  // atomic per value and block (per-lane atomics from 1024 blocks = 4800 contended adds per address,
  // which was most of this kernel's time)
  __syncthreads();
  float* red = (float*)smem;   // [4 waves][32 oc][32 k]
  const bool det = a.partial.buf != nullptr;      // deterministic way out: slot = blockIdx.x
  float* const dw = wg_base(a.dw, a.partial, (long)a.Cout * 27, blockIdx.x);
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wave * 32 + 16 * f + 4 * q + r) * 32 + 16 * g + i] = acc[f][g][r];
  __syncthreads();
  for (int e = tid; e < 32 * 32; e += 256) {
    const int oc = e >> 5, k = e & 31;
    if (k < 27 && oc < a.Cout) wg_out(dw + oc * 27 + k, (red[e] + red[1024 + e]) + (red[2048 + e] + red[3072 + e]), det);
  }
}

// bf16 training forward, tiled through LDS (round 5).  The gather kernel at the top of this file issues 8 scalar 4-byte loads per
// lane and 16-pixel group - 64 lanes x every second column of 4 (row, plane) pairs: ~20 cache lines per instruction, bound by the
// texture-address path at 2.8 TB/s.  Here a block stages the fp32 input of an 8 x 32-pixel output tile ONCE with coalesced 8-byte
// loads, as the three pre-shifted bf16 arrays A_kx[j] = x[2 (ox0 + j) + kx - pad_l] per (input row, plane) that the tiled weight
// gradient uses, and a lane gathers its 8 taps of one pixel from LDS (2-byte reads; consecutive lanes = consecutive columns).
// Persistent blocks, the next tile's loads in flight under this tile's MFMAs and stores.  Same arithmetic as the gather kernel:
// the input is rounded to bf16 once (RNE), products on the bf16 matrix core, fp32 accumulation, statistics of the fp32 values.
__global__ __launch_bounds__(256, 3) void stem_fwd_tiled_kernel(mds_stem_fwd_args a, int tiles_a, int tiles_b, int tiles_per_block) {
  MDS_CHAIN_PRIO();
  typedef bf16_t T;
  constexpr int IR = 2 * SW_ROWS + 1;                  // input rows of a tile
  constexpr int NX = IR * 3 * (SW_COLS / 8);           // x staging items: (input row, plane, 8-column group)
  __shared__ __attribute__((aligned(16))) T xa[IR * 9 * SW_PITCH + SW_PITCH];   // [IR][3 planes][3 kx][SW_PITCH] + a row of zeros
  T* zrow = xa + IR * 9 * SW_PITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = MDS_UNIFORM(tid >> 6);
  const int i = lane & 15, q = lane >> 4;
  const T* w = (const T*)a.w;
  u16x8 wf[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    if (16 * f + i < a.Cout) wf[f] = ld_frag(w + (16 * f + i) * 32 + 8 * q);
    else frag_zero(wf[f]);
  }
  if (tid < SW_PITCH) zrow[tid] = 0;
  // this lane's eight taps k = 8q + j -> (plane, ky, kx): LDS element offset of the tap's array within the tile image (row 2r of
  // the tile is added per output row r); k >= 27: the row of zeros
  int toff[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * q + j, pl = k / 9, ky = (k % 9) / 3, kx = k % 3;
    toff[j] = k < 27 ? ((ky * 3 + pl) * 3 + kx) * SW_PITCH : -1;
  }
  const long total = (long)a.N * tiles_a * tiles_b;
  long tl = (long)xcd_contiguous(blockIdx.x, gridDim.x) * tiles_per_block, tl_end = tl + tiles_per_block;
  if (tl_end > total) tl_end = total;
  float s_[8], ss_[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s_[e] = 0.f; ss_[e] = 0.f; }
  T* y = (T*)a.y;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  f32x2 rx[9];
  auto origin = [&](long t, int& img, int& oy0, int& ox0) {
    img = (int)(t / (tiles_a * tiles_b));
    const int rem = (int)(t - (long)img * tiles_a * tiles_b);
    oy0 = (rem / tiles_b) * SW_ROWS; ox0 = (rem % tiles_b) * SW_COLS;
  };
  auto issue = [&](long t) {
    int img, oy0, ox0;
    origin(t, img, oy0, ox0);
    if (tid < NX) {
      const int grp = tid & 3, pl = (tid >> 2) % 3, ir = tid / 12;
      const int iy = oy0 * 2 - a.pad_t + ir;
      const int iyc = iy < 0 ? 0 : (iy >= a.H ? a.H - 1 : iy);
      const float* row = a.x + (((long)img * 3 + pl) * a.H + iyc) * a.W;
      const int ix0 = 2 * (ox0 + 8 * grp) - a.pad_l;
      if (iy >= 0 && iy < a.H && ix0 >= 0 && ix0 + 17 < a.W) {   // interior: nine 8-byte loads
#pragma unroll
        for (int j = 0; j < 9; ++j) rx[j] = *(const f32x2*)(row + ix0 + 2 * j);
      } else {
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          const int ix = ix0 + 2 * j;
          const bool ok0 = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W, ok1 = iy >= 0 && iy < a.H && ix + 1 >= 0 && ix + 1 < a.W;
          const int c0 = ix < 0 ? 0 : (ix >= a.W ? a.W - 1 : ix), c1 = ix + 1 < 0 ? 0 : (ix + 1 >= a.W ? a.W - 1 : ix + 1);
          const float v0 = row[c0], v1 = row[c1];
          rx[j] = (f32x2){ok0 ? v0 : 0.f, ok1 ? v1 : 0.f};
        }
      }
    }
  };
  if (tl < tl_end) issue(tl);
  for (; tl < tl_end; ++tl) {
    __syncthreads();                                   // the previous tile's fragments have been read
    if (tid < NX) {
      const int grp = tid & 3, pl = (tid >> 2) % 3, ir = tid / 12;
      T* base = xa + ((ir * 3 + pl) * 3) * SW_PITCH + 8 * grp;
      float v0[8], v1[8], v2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { v0[j] = rx[j][0]; v1[j] = rx[j][1]; v2[j] = rx[j + 1][0]; }
      store8(base, v0); store8(base + SW_PITCH, v1); store8(base + 2 * SW_PITCH, v2);
    }
    __syncthreads();
    if (tl + 1 < tl_end) issue(tl + 1);
    int img, oy0, ox0;
    origin(tl, img, oy0, ox0);
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int r = 2 * wave + rr, oy = oy0 + r;       // output row of the tile handled by this wave
#pragma unroll
      for (int h = 0; h < 2; ++h) {                    // its two 16-pixel groups
        const int col = 16 * h + i, ox = ox0 + col;
        const T* rowp = xa + (2 * r) * 9 * SW_PITCH + col;
        u16x8 xf;
#pragma unroll
        for (int j = 0; j < 8; ++j) xf[j] = toff[j] >= 0 ? rowp[toff[j]] : zrow[0];
        f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
        mma16(wf[0], xf, acc[0]);                      // acc[r] = y[pixel i][oc = 4q + r]
        mma16(wf[1], xf, acc[1]);
        if (oy < a.OH && ox < a.OW) {
          const long row = ((long)img * a.OH + oy) * a.OW + ox;
#pragma unroll
          for (int f = 0; f < 2; ++f) {
            const int oc = 16 * f + 4 * q;
            if (oc < a.Cout) {
              float v[4] = {acc[f][0], acc[f][1], acc[f][2], acc[f][3]};
              store4(y + row * a.Cout + oc, v);
#pragma unroll
              for (int e = 0; e < 4; ++e) { s_[f * 4 + e] += v[e]; ss_[f * 4 + e] += v[e] * v[e]; }
            }
          }
        }
      }
    }
  }
  if (a.stats) {
    double* st = a.stats + (long)(blockIdx.x % MDS_STAT_SLOTS) * 2 * a.Cout;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float s = sum_over_i16(s_[e]), ss = sum_over_i16(ss_[e]);
      const int oc = 16 * (e >> 2) + 4 * q + (e & 3);
      if (i == 0 && oc < a.Cout) { atomicAdd(st + oc, (double)s); atomicAdd(st + a.Cout + oc, (double)ss); }
    }
  }
}

static int stem_fwd_tiled(const mds_stem_fwd_args* a, mds_stream_t stream) {
  const int tiles_a = cdiv(a->OH, SW_ROWS), tiles_b = cdiv(a->OW, SW_COLS);
  const long total = (long)a->N * tiles_a * tiles_b;
  const int tpb = (int)cdiv(total, total < 768 ? total : 768);   // three blocks per CU
  MDS_LAUNCH(stem_fwd_tiled_kernel, dim3(cdiv(total, tpb)), dim3(256), 0, stream, *a, tiles_a, tiles_b, tpb);
  return mds_check_launch("stem_fwd");
}

// launch geometry of mds_stem_wgrad: the launcher and the partial-buffer query both come here
struct StemWgGeo { int tiles_a, tiles_b, tpb; long blocks, slots; };
static StemWgGeo stem_wgrad_geo(const mds_stem_wgrad_args* a) {
  StemWgGeo g = {};
  if (a->dtype == MDS_BF16) {
    g.tiles_a = cdiv(a->OH, SW_ROWS); g.tiles_b = cdiv(a->OW, SW_COLS);
    const long total = (long)a->N * g.tiles_a * g.tiles_b;
    g.tpb = (int)cdiv(total, total < 768 ? total : 768);   // three blocks per CU
    g.blocks = g.slots = cdiv(total, g.tpb);               // a block's four waves meet in LDS: one slot per block
  } else {
    const long ngroups = (long)a->N * a->OH * ((a->OW + 31) / 32);
    g.blocks = (ngroups + 3) / 4;
    if (g.blocks > 512) g.blocks = 512;
    g.slots = 4 * g.blocks;                                // one slot per wave
  }
  return g;
}
#define STEM_WGRAD_DIMS_OK(a) \
  MDS_REQUIRE(a && a->N > 0 && a->H > 0 && a->W > 0 && a->OH > 0 && a->OW > 0, "stem_wgrad: bad dims"); \
  MDS_REQUIRE(a->Cout % 16 == 0 && a->Cout <= 32, "stem_wgrad: Cout=%d must be 16 or 32", a->Cout)
extern "C" long mds_stem_wgrad_partial_floats(const mds_stem_wgrad_args* a) {
  STEM_WGRAD_DIMS_OK(a);
  return wg_floats((long)a->Cout * 27, stem_wgrad_geo(a).slots);
}
extern "C" int mds_stem_wgrad(const mds_stem_wgrad_args* a, mds_stream_t stream) {
  STEM_WGRAD_DIMS_OK(a);
  const StemWgGeo sg = stem_wgrad_geo(a);
  MDS_PARTIAL_OK(a->partial, wg_floats((long)a->Cout * 27, sg.slots), "stem_wgrad");
  const bool dyp = a->dyp.mode != 0;
  MDS_REQUIRE(a->x && (a->dy || dyp) && a->dw, "stem_wgrad: null pointer");
  if (dyp) {
    MDS_REQUIRE(a->dtype == MDS_BF16, "stem_wgrad: the dy prologue is a bf16 feature");
    MDS_REQUIRE(a->dyp.g.u && a->dyp.y && a->dyp.bn && a->dyp.lin && (a->dyp.g.mode == MDS_G_PLAIN || a->dyp.g.mode == MDS_G_SILU),
                "stem_wgrad: dy prologue needs u, y, bn, lin and a PLAIN or SILU gradient source");
  }
  if (a->dtype == MDS_BF16) {
    const int tiles_a = sg.tiles_a, tiles_b = sg.tiles_b, tpb = sg.tpb;
    const size_t smem = (size_t)((2 * SW_ROWS + 1) * 9 + SW_ROWS * SW_COLS + 1) * SW_PITCH * sizeof(bf16_t);
    if (dyp) MDS_LAUNCH(stem_wgrad_tiled_kernel<true>, dim3((unsigned)sg.blocks), dim3(256), smem, stream, *a, tiles_a, tiles_b, tpb);
    else MDS_LAUNCH(stem_wgrad_tiled_kernel<false>, dim3((unsigned)sg.blocks), dim3(256), smem, stream, *a, tiles_a, tiles_b, tpb);
  } else {   // the gather kernel exists for fp32 alone
    if (a->dtype != MDS_F32) { mds_set_error("unsupported dtype %d", (int)a->dtype); return MDS_ERR_UNSUPPORTED; }
    MDS_LAUNCH(stem_wgrad_kernel<float>, dim3((unsigned)sg.blocks), dim3(256), 0, stream, *a);
  }
  if (int rc = mds_check_launch("stem_wgrad")) return rc;
  return wg_finish(a->partial, a->dw, (long)a->Cout * 27, sg.slots, stream);
}

// ---- data gradient: dx[n][p][iy][ix] = sum_{ky,kx} sum_o w[o][p][ky][kx] * dy[n][(iy + pad_t - ky) / 2][(ix + pad_l - kx) / 2][o] over the
// taps whose two divisions are exact and land inside dy - the transposed stride-2 convolution, 32 -> 3, written as a GATHER: no
// atomics, every dx element stored once.  In a = iy + pad_t, b = ix + pad_l the parity decides the taps: an even a takes ky = 0
// (dy row a/2) and ky = 2 (row a/2 - 1), an odd a takes ky = 1 (row (a-1)/2); columns alike.  So the 2 x 2 patch (2A..2A+1, 2B..2B+1)
// reads dy rows A-1, A and columns B-1, B, and every filter value is used exactly once per patch: 864 FMAs for 12 outputs.
// A thread owns 2 rows x 4 columns x 3 planes (two patches side by side: one 16-byte store per plane and row); a block of
// SdCfg::rows x 32 threads stages its (rows + 1) x 65 dy pixels ONCE into LDS - zeros outside dy, so the edge rules need no
// branch in the arithmetic - in the storage type (a dy formed on load, A*g + B*y + D, is rounded to it: what mds_bn_bwd_apply would
// have written).  In a tile row the even dy columns come first, then the odd ones: neighbouring lanes then read neighbouring LDS
// pixels (pitch 80 B / 144 B: the sixteen lanes of a ds_read_b128 group hit sixteen different 16-byte bank groups).  The filter is
// read through the scalar cache (wave-uniform index), an FMA takes it as its scalar operand.  Streaming: 64 B in and 48 B out per
// patch against 864 FMAs.  Order of the sum of one element: o ascending, inside one o ky ascending, then kx - fixed, so two runs
// give the same bits.
#define SD_COLS 32
template <typename T> struct SdCfg;
template <> struct SdCfg<bf16_t> { static const int rows = 8, pitch = 40; };
template <> struct SdCfg<float> { static const int rows = 4, pitch = 36; };
template <typename T> MDS_DEV float stem_w(const T* w, int idx);      // w[idx] of the MDS_PACK_STEM filter, idx wave-uniform
template <> MDS_DEV float stem_w<float>(const float* w, int idx) { return ld_uniform(w, idx); }
template <> MDS_DEV float stem_w<bf16_t>(const bf16_t* w, int idx) {
  const uint32_t pair = f2bits(ld_uniform((const float*)w, idx >> 1));
  return bits2f((idx & 1) ? (pair & 0xffff0000u) : (pair << 16));
}

template <typename T, bool DYP>
__global__ __launch_bounds__(SdCfg<T>::rows * SD_COLS) void stem_dgrad_kernel(mds_stem_dgrad_args a, int tiles_a, int tiles_b, int vec) {
  MDS_CHAIN_PRIO();
  constexpr int TR = SdCfg<T>::rows, NT = TR * SD_COLS, PITCH = SdCfg<T>::pitch;
  constexpr int NC = 2 * SD_COLS + 1, NE = SD_COLS + 1;      // dy columns of a tile, the even ones of them
  constexpr int NPX = (TR + 1) * NC;
  constexpr int BATCH = 4;                                   // 16-byte loads a thread keeps in flight (twice that with DYP)
  __shared__ __attribute__((aligned(16))) T dys[NPX * PITCH];
  const int tid = threadIdx.x;
  const int csh = a.Cout == 32 ? 2 : 1, ch = tid & ((1 << csh) - 1);      // 8-channel chunks per pixel = 1 << csh; this thread's chunk
  const long t = xcd_contiguous(blockIdx.x, gridDim.x);     // neighbouring tiles share a halo row / column: same XCD, same L2
  const int img = (int)(t / (tiles_a * tiles_b));
  const int rem = (int)(t - (long)img * tiles_a * tiles_b);
  const int A0 = (rem / tiles_b) * TR, J0 = (rem % tiles_b) * SD_COLS;
  const int oy0 = A0 - 1, ox0 = 2 * J0 - 1;                  // dy pixel of tile position (0, 0)
  const T* src = (const T*)(DYP ? a.dyp.g.u : a.dy);
  const T* ysrc = (const T*)a.dyp.y;                         // the BatchNorm input y has u's layout
  float cA[8], cB[8], cD[8], csc[8], cshf[8];
  if (DYP) {
    const int c = 8 * ch, C = a.Cout;
    load8f(a.dyp.lin + c, cA); load8f(a.dyp.lin + C + c, cB); load8f(a.dyp.lin + 2 * C + c, cD);
    load8f(a.dyp.bn + c, csc); load8f(a.dyp.bn + C + c, cshf);
  }
  const bool gsilu = DYP && a.dyp.g.mode == MDS_G_SILU;
  const int nitems = NPX << csh;
  for (int base = 0; base < nitems; base += BATCH * NT) {
    RawV8<T> ru[BATCH], ry[DYP ? BATCH : 1];
    unsigned ok = 0;
#pragma unroll
    for (int k = 0; k < BATCH; ++k) {
      const int it = base + k * NT + tid, px = it >> csh, r = px / NC, c = px - r * NC;
      const int oy = oy0 + r, ox = ox0 + c;
      const bool in = it < nitems && oy >= 0 && oy < a.OH && ox >= 0 && ox < a.OW;
      const long off = ((((long)img * a.OH + oy) * a.OW + ox) << (csh + 3)) + 8 * ch;
      if (in) ru[k].ld(src + off);
      else ru[k].zero();
      if (DYP) {
        if (in) ry[k].ld(ysrc + off);
        else ry[k].zero();
      }
      ok |= (in ? 1u : 0u) << k;
    }
#pragma unroll
    for (int k = 0; k < BATCH; ++k) {
      const int it = base + k * NT + tid, px = it >> csh, r = px / NC, c = px - r * NC;
      if (it < nitems) {
        T* dst = dys + (r * NC + ((c & 1) ? NE + (c >> 1) : (c >> 1))) * PITCH + 8 * ch;
        if (!DYP) {
          ru[k].st(dst);
        } else {
          float u[8], yv[8], v[8];
          ru[k].get(u);
          ry[k].get(yv);
          const bool in = (ok >> k) & 1u;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float g = u[e];
            if (gsilu) g *= silu_gradf_(yv[e] * csc[e] + cshf[e]);
            v[e] = in ? cA[e] * g + cB[e] * yv[e] + cD[e] : 0.f;      // positions outside dy contribute nothing (D != 0)
          }
          store8(dst, v);
        }
      }
    }
  }
  __syncthreads();
  const int ta = tid / SD_COLS, tj = tid % SD_COLS;
  const int iy0 = 2 * (A0 + ta) - a.pad_t, ix0 = 4 * (J0 + tj) - a.pad_l;    // first of this thread's 2 rows / 4 columns
  if (iy0 < a.H && ix0 < a.W) {
    const T* w = (const T*)a.w;
    float acc[3][2][4];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) acc[p][ra][bb] = 0.f;
    const T* lds0 = dys + (ta * NC + tj) * PITCH;             // dy row A-1, column 2B-1 of the left patch
    for (int oc = 0; oc < a.Cout; oc += 8) {
      float d[2][3][8];                                        // [row A-1, A][column 2B-1, 2B, 2B+1][channel]
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const T* rowp = lds0 + r * NC * PITCH + oc;
        load8(rowp, d[r][0]);
        load8(rowp + NE * PITCH, d[r][1]);
        load8(rowp + PITCH, d[r][2]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int wb = (oc + e) * 32;
        float wc[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) wc[k] = stem_w<T>(w, wb + k);
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
              const float wv = wc[p * 9 + ky * 3 + kx];
              const int ra = ky == 1 ? 1 : 0, r = ky == 2 ? 0 : 1, rb = kx == 1 ? 1 : 0;
#pragma unroll
              for (int q = 0; q < 2; ++q) {                    // the two patches
                const int cc = kx == 2 ? q : q + 1;
                acc[p][ra][2 * q + rb] = fmaf(wv, d[r][cc][e], acc[p][ra][2 * q + rb]);
              }
            }
      }
    }
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int ra = 0; ra < 2; ++ra) {
        const int iy = iy0 + ra;
        if (iy < 0 || iy >= a.H) continue;
        float* row = a.dx + (((long)img * 3 + p) * a.H + iy) * a.W;
        if (vec) {                                             // W % 4 == 0, pad_l == 0, dx 16-byte aligned: ix0 .. ix0 + 3 are inside
          store4(row + ix0, acc[p][ra]);
        } else {
#pragma unroll
          for (int bb = 0; bb < 4; ++bb)
            if (ix0 + bb >= 0 && ix0 + bb < a.W) row[ix0 + bb] = acc[p][ra][bb];
        }
      }
  }
}

extern "C" long mds_stem_dgrad(const mds_stem_dgrad_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a && a->N > 0 && a->H > 0 && a->W > 0 && a->OH > 0 && a->OW > 0, "stem_dgrad: bad dims");
  MDS_REQUIRE(a->Cout % 16 == 0 && a->Cout > 0 && a->Cout <= 32, "stem_dgrad: Cout=%d must be 16 or 32", a->Cout);
  MDS_REQUIRE(a->pad_t >= 0 && a->pad_t <= 1 && a->pad_l >= 0 && a->pad_l <= 1, "stem_dgrad: pad_t=%d, pad_l=%d must be 0 or 1", a->pad_t, a->pad_l);
  const bool dyp = a->dyp.mode != 0;
  MDS_REQUIRE(a->w && (a->dy || dyp) && a->dx, "stem_dgrad: null pointer");
  if (dyp) {
    MDS_REQUIRE(a->dyp.mode == 1 && a->dyp.g.u && a->dyp.y && a->dyp.bn && a->dyp.lin && (a->dyp.g.mode == MDS_G_PLAIN || a->dyp.g.mode == MDS_G_SILU),
                "stem_dgrad: dy prologue needs u, y, bn, lin and a PLAIN or SILU gradient source");
    MDS_REQUIRE((((uintptr_t)a->dyp.g.u | (uintptr_t)a->dyp.y | (uintptr_t)a->dyp.bn | (uintptr_t)a->dyp.lin) & 15) == 0,
                "stem_dgrad: u, y, bn and lin must be 16-byte aligned");
  } else {
    MDS_REQUIRE(((uintptr_t)a->dy & 15) == 0, "stem_dgrad: dy must be 16-byte aligned");
  }
  MDS_REQUIRE(((uintptr_t)a->w & 3) == 0 && ((uintptr_t)a->dx & 3) == 0, "stem_dgrad: w and dx must be 4-byte aligned");
  const int vec = (a->W % 4 == 0 && a->pad_l == 0 && ((uintptr_t)a->dx & 15) == 0) ? 1 : 0;
  const int rows = a->dtype == MDS_BF16 ? SdCfg<bf16_t>::rows : SdCfg<float>::rows;
  const int tiles_a = cdiv(cdiv(a->H + a->pad_t, 2), rows), tiles_b = cdiv(cdiv(a->W + a->pad_l, 4), SD_COLS);
  const long total = (long)a->N * tiles_a * tiles_b;
  MDS_REQUIRE(total < (1L << 31), "stem_dgrad: %ld tiles", total);
  MDS_DISPATCH_DTYPE(a->dtype, T, {
    if (dyp) MDS_LAUNCH((stem_dgrad_kernel<T, true>), dim3((unsigned)total), dim3(SdCfg<T>::rows * SD_COLS), 0, stream, *a, tiles_a, tiles_b, vec);
    else MDS_LAUNCH((stem_dgrad_kernel<T, false>), dim3((unsigned)total), dim3(SdCfg<T>::rows * SD_COLS), 0, stream, *a, tiles_a, tiles_b, vec);
  });
  return mds_check_launch("stem_dgrad");
}
