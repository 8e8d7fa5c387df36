// k_c3p.hip — the dense 3x3 forward with the 1x1 projection that follows it as its tail (inference plans, mds_project_t).
//
// An edge-residual block's expanded tensor ya = silu(bn1(conv3x3(x))) only feeds the 1x1 projection behind it, pixel by
// pixel: the tile of ya a block has just produced is exactly the operand of the projection for the same pixels (no halo).
// A block owns a tile of 4·MF x 16 output pixels (wave w: rows MF·w .. MF·w + MF - 1, a 16-pixel row per MFMA tile):
//   1. the input patch of the tile is staged in LDS ONCE, all Cin channels;
//   2. `mid` (= Cout of the 3x3) is walked CP_CH = 32 channels at a time.  Per chunk the 32 filter rows [32][9·Cin] and the
//      chunk's 32 columns of the projection filter are staged in LDS (from L2: the filters are small and shared by every
//      block), the 3x3 is an MFMA implicit GEMM into acc[MF][2] as in conv_fwd_q_kernel, and BN1 + SiLU run in registers;
//   3. the activated chunk never leaves the registers: with A = filter rows and B = pixels, lane (i, q) of the first product
//      holds channels 4q .. 4q+3 of both 16-channel halves for pixel i - eight k values of column i.  The MFMA sums over k
//      in any order as long as both operands agree, so those eight values ARE the lane's B fragment of the second product
//      under the k order (q, j) -> channel 16·(j / 4) + 4q + j % 4, and the A fragment (projection filter, from LDS) is read
//      in the same order: two 4-element reads per lane.  No LDS round trip, no bank-conflict question for the activation;
//   4. out[MF][cout / 16] accumulates over all chunks in registers; after the last: BN2 (+ residual), whole-pixel stores.
// LDS (fp32, Cin 48, stride 1): patch 6·18·224 B = 24 KiB (4 x 16 tile; 71 KiB at 16 x 16) + slab 32·1824 B = 57 KiB + projection
// 7.5 KiB.  The 3x3 filter is re-staged by every tile (it does not fit beside the patch beyond blocks.1.0): DESIGN 10.2 has the L2
// traffic this costs and the measurement (faster than the two launches it replaces on all four blocks).
#include "gemm.h"

#define CP_TB 16   // tile width (pixels of one MFMA column block)
#define CP_CH 32   // mid channels per chunk = one k step of the second product

// LDS row pitch (elements): the next byte pitch that is 32 (mod 64) - conflict-free for ds_read_b128 (as k_conv.hip)
MDS_DEV int cp_pitch(int elems, int esz) { const int b = elems * esz; return (b + ((96 - b % 64) % 64)) / esz; }
static inline int cp_pitch_h(int elems, int esz) { const int b = elems * esz; return (b + ((96 - b % 64) % 64)) / esz; }

struct CpGeom {
  int dymin, dxmin, TH, TW, tiles_a, tiles_b, KS;
};

// eight k values of one filter row in the second product's k order: 4 consecutive elements at p and 4 at p + 16
MDS_DEV u16x8 cp_ld44(const bf16_t* p) {
  const u16x4 a = *(const u16x4*)p, b = *(const u16x4*)(p + 16);
  return (u16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
MDS_DEV f32x8 cp_ld44(const float* p) {
  const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 16);
  return (f32x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

template <typename T, int IS, int MF, int CF, bool X3>
__global__ __launch_bounds__(256, 2) void conv_project_kernel(mds_conv_fwd_args a, CpGeom gq) {
  MDS_CHAIN_PRIO();
  typedef Mma<T, X3> MM;
  constexpr int TA = 4 * MF;
  MDS_DYN_SMEM(smem);
  const int Cin = a.Cin, mid = a.Cout, cout = a.project.cout, K = a.ntaps * Cin, KS = gq.KS, TW = gq.TW;
  const int LDX = cp_pitch(Cin, sizeof(T)), LDW = cp_pitch(KS * 32, sizeof(T)), LDP = cp_pitch(CP_CH, sizeof(T));
  const int npix = gq.TH * TW, cpp = Cin >> 3, nitems = npix * cpp;
  const int nch = (mid + CP_CH - 1) / CP_CH, midp = nch * CP_CH;
  T* xs = (T*)smem;                              // [npix][LDX] input patch, all channels
  T* ws = xs + npix * LDX;                       // [CP_CH][LDW] filter rows of the current chunk
  T* ps = ws + CP_CH * LDW;                      // [16 * CF][LDP] projection filter, columns of the current chunk
  float* pes = (float*)(ps + 16 * CF * LDP);     // [midp] output transform of the 3x3 (zeros past mid)
  float* peh = pes + midp;
  int* ktab = (int*)(peh + midp);                // [KS * 4] LDS offset (tap shift + channel) of each 8-wide k chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = MDS_UNIFORM(tid >> 6);
  const int i = lane & 15, q = lane >> 4;
  const T* w = (const T*)a.w;
  const T* w2 = (const T*)a.project.w;

  // consecutive tiles (shared halo rows) on one XCD
  const int tiles_ab = gq.tiles_a * gq.tiles_b;
  const long t = (long)xcd_contiguous(blockIdx.x, gridDim.x);
  const int img = (int)(t / tiles_ab), rem = (int)(t - (long)img * tiles_ab);
  const int a0 = (rem / gq.tiles_b) * TA, b0 = (rem % gq.tiles_b) * CP_TB;

  for (int c = tid; c < KS * 4; c += 256) {
    const int k = 8 * c;
    int off = 0;
    if (k < K) {
      const int tp = k / Cin, ch = k - tp * Cin;
      off = ((a.dy[tp] - gq.dymin) * TW + (a.dx[tp] - gq.dxmin)) * LDX + ch;
    }
    ktab[c] = off;
  }
  for (int c = tid; c < midp; c += 256) {
    pes[c] = c < mid ? a.epi.scale[c] : 0.f;
    peh[c] = c < mid ? a.epi.shift[c] : 0.f;
  }
  {
    const T* x = (const T*)a.x + (long)img * a.IH * a.IW * Cin;
    const float rTW = 1.0f / (float)TW, rcpp = 1.0f / (float)cpp;
    for (int it = tid; it < nitems; it += 256) {
      const int pix = fdiv(it, rcpp), c8 = it - pix * cpp;
      const int ty = fdiv(pix, rTW), tx = pix - ty * TW;
      const int iy = a0 * IS + gq.dymin + ty, ix = b0 * IS + gq.dxmin + tx;
      RawV8<T> r;
      r.zero();                                  // zero padding of x
      if (iy >= 0 && iy < a.IH && ix >= 0 && ix < a.IW) r.ld(x + ((long)iy * a.IW + ix) * Cin + 8 * c8);
      r.st(xs + pix * LDX + 8 * c8);
    }
  }
  int xbase[MF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) xbase[mf] = ((MF * wave + mf) * IS * TW + i * IS) * LDX;
  const int wbase = i * LDW + 8 * q;
  const bool silu = a.epi.mode == MDS_EPI_BN_SILU;

  f32x4 out[MF][CF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int cf = 0; cf < CF; ++cf) out[mf][cf] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int ch = 0; ch < nch; ++ch) {
    const int m0 = ch * CP_CH;
    if (ch) __syncthreads();                     // the previous chunk's fragment reads are done
    for (int e = tid; e < CP_CH * KS * 4; e += 256) {
      const int n = e / (KS * 4), c = e - n * (KS * 4), k = 8 * c;
      RawV8<T> r;
      r.zero();
      if (m0 + n < mid && k < K) {
        const int tp = k / Cin, cc = k - tp * Cin;
        r.ld(w + ((long)(m0 + n) * a.wtaps + a.wi[tp]) * Cin + cc);
      }
      r.st(ws + n * LDW + k);
    }
    for (int e = tid; e < 16 * CF * 4; e += 256) {
      const int c = e >> 2, j8 = (e & 3) * 8;
      RawV8<T> r;
      r.zero();
      if (c < cout && m0 + j8 < mid) r.ld(w2 + (long)c * mid + m0 + j8);
      r.st(ps + c * LDP + j8);
    }
    __syncthreads();                             // (first pass: patch + tables staged as well)

    // ---- 3x3: acc[mf][nf] = filter rows m0 + 16 nf .. (A) x the patch (B); lane (i, q): channels 4q .. 4q+3, pixel i
    f32x4 acc[MF][2];
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) { acc[mf][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[mf][1] = acc[mf][0]; }
    int xo_next = ktab[q];
    for (int s = 0; s < KS; ++s) {
      const int xo = xo_next;                    // the tap-offset lookup of step s + 1 is issued a step ahead
      xo_next = ktab[4 * (s + 1 < KS ? s + 1 : s) + q];
      typename MM::frag xf[MF], wf[2];
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) xf[mf] = MM::prep(ld_frag(xs + xbase[mf] + xo));
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) wf[nf] = MM::prep(ld_frag(ws + wbase + 16 * nf * LDW + 32 * s));   // rows past mid are zeros
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) MM::mma(wf[nf], xf[mf], acc[mf][nf]);
    }

    // ---- BN1 + activation in registers, then out[mf][cf] += projection rows 16 cf .. (A) x the activated chunk (B)
    const f32x4 es0 = *(const f32x4*)(pes + m0 + 4 * q), eh0 = *(const f32x4*)(peh + m0 + 4 * q);
    const f32x4 es1 = *(const f32x4*)(pes + m0 + 16 + 4 * q), eh1 = *(const f32x4*)(peh + m0 + 16 + 4 * q);
    typename MM::frag pf[CF];
#pragma unroll
    for (int cf = 0; cf < CF; ++cf) pf[cf] = MM::prep(cp_ld44(ps + (16 * cf + i) * LDP + 4 * q));
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z0 = acc[mf][0][r] * es0[r] + eh0[r], z1 = acc[mf][1][r] * es1[r] + eh1[r];
        v[r] = silu ? siluf_(z0) : z0;           // channels past mid: acc = scale = shift = 0 -> 0 either way
        v[4 + r] = silu ? siluf_(z1) : z1;
      }
      typename Frag<T>::type f;
      frag_from8(f, v);                          // bf16: rounded once, as the stored ya of the two-launch form
      const typename MM::frag yf = MM::prep(f);
#pragma unroll
      for (int cf = 0; cf < CF; ++cf) MM::mma(pf[cf], yf, out[mf][cf]);
    }
  }

  // ---- BN2 (+ residual), store: lane (i, q) holds channels 16 cf + 4q .. + 3 of pixel (a0 + MF wave + mf, b0 + i)
  T* y = (T*)a.y;
  const T* res = (const T*)a.residual;
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int aa = a0 + MF * wave + mf, bb = b0 + i;
    const bool valid = aa < a.A && bb < a.B;
    const long row = ((long)img * a.OH + (a.oy0 + aa)) * a.OW + (a.ox0 + bb);
#pragma unroll
    for (int cf = 0; cf < CF; ++cf) {
      const int n = 16 * cf + 4 * q;
      if (valid && n < cout) {
        float v[4], rs[4] = {0.f, 0.f, 0.f, 0.f};
        if (res) load4(res + row * cout + n, rs);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = out[mf][cf][r] * a.project.scale[n + r] + a.project.shift[n + r] + rs[r];
        store4(y + row * cout + n, v);
      }
    }
  }
}

static int cp_tap_extent(const int* d, int n, int* dmin) {
  int lo = d[0], hi = d[0];
  for (int t = 1; t < n; ++t) { if (d[t] < lo) lo = d[t]; if (d[t] > hi) hi = d[t]; }
  *dmin = lo;
  return hi - lo;
}

// mds_conv_fwd with a->project.w set (k_conv.hip routes here after its own argument checks)
int conv_fwd_project(const mds_conv_fwd_args* a, mds_stream_t stream) {
  const mds_project_t& p = a->project;
  MDS_REQUIRE(a->epi.mode == MDS_EPI_AFFINE || a->epi.mode == MDS_EPI_BN_SILU, "conv_fwd (project): needs an output transform of the 3x3 (epi)");
  MDS_REQUIRE(a->pro.mode == MDS_PRO_NONE && !a->stats && a->post.mode == MDS_POST_NONE, "conv_fwd (project): no prologue, no statistics, no post statistics");
  MDS_REQUIRE(a->ngroups <= 1, "conv_fwd (project): no tap groups");
  MDS_REQUIRE(a->os == 1, "conv_fwd (project): os == 1 (a forward convolution)");
  MDS_REQUIRE(p.scale && p.shift, "conv_fwd (project): null scale / shift");
  MDS_REQUIRE(p.cout > 0 && p.cout % 16 == 0 && p.cout <= MDS_PROJECT_COUT_MAX, "conv_fwd (project): cout=%d needs %% 16 == 0 and <= %d", p.cout, MDS_PROJECT_COUT_MAX);
  MDS_REQUIRE(a->Cout <= MDS_PROJECT_MID_MAX && a->Cin <= MDS_PROJECT_CIN_MAX, "conv_fwd (project): Cout=%d <= %d, Cin=%d <= %d", a->Cout, MDS_PROJECT_MID_MAX,
              a->Cin, MDS_PROJECT_CIN_MAX);
  for (int t = 0; t < a->ntaps; ++t) MDS_REQUIRE(a->wi[t] >= 0 && a->wi[t] < a->wtaps, "conv_fwd (project): tap %d reads filter tap %d of %d", t, a->wi[t], a->wtaps);
  int dymin, dxmin;
  const int eh = cp_tap_extent(a->dy, a->ntaps, &dymin), ew = cp_tap_extent(a->dx, a->ntaps, &dxmin);
  const int KS = cdiv(a->ntaps * a->Cin, 32), esz = a->dtype == MDS_BF16 ? 2 : 4, CF = p.cout / 16;
  const int midp = cdiv(a->Cout, CP_CH) * CP_CH;
  // tile height 4 MF: the tallest that (in this order of preference) gives every CU a tile and lets two blocks share a CU's LDS;
  // short of tiles (blocks.2.1 of one 736 x 1280 image is 60 tiles of 16 x 16), the smallest that fits - more, smaller blocks
  const int mf_try[3] = {a->is == 1 ? 4 : 2, a->is == 1 ? 2 : 1, a->is == 1 ? 1 : 0};
  const long cus = mds_cu_count();
  int MFs = 0, THq = 0, TWq = 0, best = -1;
  size_t smem = 0;
  for (int mi = 0; mi < 3; ++mi) {
    const int mf = mf_try[mi];
    if (!mf) continue;
    const int th = (4 * mf - 1) * a->is + eh + 1, tw = (CP_TB - 1) * a->is + ew + 1;
    const size_t sm = ((size_t)th * tw * cp_pitch_h(a->Cin, esz) + (size_t)CP_CH * cp_pitch_h(KS * 32, esz) + (size_t)16 * CF * cp_pitch_h(CP_CH, esz)) * esz +
                      2 * (size_t)midp * sizeof(float) + (size_t)KS * 16;
    if (sm > (size_t)160 * 1024) continue;
    const long tiles = (long)a->N * cdiv(a->A, 4 * mf) * cdiv(a->B, CP_TB);
    const int score = (tiles >= cus ? 2 : 0) + (sm <= (size_t)80 * 1024 ? 1 : 0);   // ties: the taller tile (tried first) while every CU has one, else the smaller
    if (score > best || (score == best && tiles < cus)) { best = score; MFs = mf; THq = th; TWq = tw; smem = sm; }
  }
  MDS_REQUIRE(MFs, "conv_fwd (project): the input patch + a filter slab do not fit in LDS (Cin=%d, taps span %d x %d)", a->Cin, eh + 1, ew + 1);
  CpGeom gq;
  gq.dymin = dymin; gq.dxmin = dxmin; gq.TH = THq; gq.TW = TWq; gq.KS = KS;
  gq.tiles_a = cdiv(a->A, 4 * MFs); gq.tiles_b = cdiv(a->B, CP_TB);
  const long total = (long)a->N * gq.tiles_a * gq.tiles_b;
  MDS_REQUIRE(total < 2147483647L, "conv_fwd (project): grid");
  const dim3 grid((unsigned)total), block(256);
  // (fp32 in split-bf16 products unless the library is built with -DMDS_EVAL_X3=0: a compile-time choice, one instantiation per type)
#define CP_GO3(T, IS_, MF_, CF_) MDS_LAUNCH((conv_project_kernel<T, IS_, MF_, CF_, (sizeof(T) == 4 && MDS_EVAL_X3)>), grid, block, smem, stream, *a, gq)
#define CP_GO2(T, IS_, MF_) do { if (CF == 1) CP_GO3(T, IS_, MF_, 1); else if (CF == 2) CP_GO3(T, IS_, MF_, 2); else CP_GO3(T, IS_, MF_, 3); } while (0)
#define CP_GO(T)                                                 \
  do {                                                           \
    if (a->is == 1 && MFs == 4) CP_GO2(T, 1, 4);                 \
    else if (a->is == 1 && MFs == 2) CP_GO2(T, 1, 2);            \
    else if (a->is == 1) CP_GO2(T, 1, 1);                        \
    else if (MFs == 2) CP_GO2(T, 2, 2);                          \
    else CP_GO2(T, 2, 1);                                        \
  } while (0)
  MDS_DISPATCH_DTYPE(a->dtype, T, CP_GO(T));
#undef CP_GO
#undef CP_GO2
#undef CP_GO3
  return mds_check_launch("conv_fwd (project)");
}
