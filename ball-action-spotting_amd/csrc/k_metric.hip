// k_metric.hip — epoch metrics on the device (mds_metric_push, mds_metric_eval, include/mds.h; reference src/metrics.py):
// one launch per step appends the step's (B, C) predictions and targets to the epoch buffers; at the end of a phase two
// launches give every class's average precision and binary accuracy.  Nothing returns to the host in between.
//
// Average precision without a sort: a positive row's precision is tp_j / n_j with n_j, tp_j counted over all rows by fp32
// compares - O(N^2 / 4 .. N^2) compares per class, VALU-bound (about four VALU instructions per pair of rows), fed by broadcast LDS reads
// (every lane of a wave reads the same 16 bytes: one LDS cycle per group, no conflicts).  A tile is 256 rows x 2 floats = 2 KB,
// double-buffered: one barrier per tile.  The sums are taken in a fixed order by one thread: no floating-point atomics.
#include "platform.h"

// the header's arithmetic contract: every quotient and every sum is rounded on its own
#pragma clang fp contract(off)

#define MET_T MDS_METRIC_TILE

// the workspace, class-major: S[C][tiles] doubles, then positives[C][tiles] and hits[C][tiles] (int32)
struct MetWs { double* S; int* pos; int* hit; };
MDS_DEV MetWs met_ws(void* base, long tiles, int C, int c) {
  MetWs w;
  w.S = (double*)base + c * tiles;
  int* ib = (int*)((double*)base + C * tiles);
  w.pos = ib + c * tiles;
  w.hit = ib + (C + c) * tiles;
  return w;
}

MDS_DEV bool met_finite(float v) { return (f2bits(v) & 0x7f800000u) != 0x7f800000u; }

// ------------------------------------------------------------------ push: one step's rows
template <typename T>
__global__ __launch_bounds__(256) void metric_push_kernel(mds_metric_push_args a) {
  __shared__ int s_bad[2];
  const int tid = threadIdx.x, n = a.B * a.C;
  if (tid < 2) s_bad[tid] = 0;
  __syncthreads();
  const T* pred = (const T*)a.pred;
  float* dp = a.dst_pred + a.row * a.C;
  float* dt = a.dst_target + a.row * a.C;
  int soft = 0, wild = 0;
  for (unsigned e = blockIdx.x * 256u + tid; e < (unsigned)n; e += gridDim.x * 256u) {      // (n < 2^31: no wrap)
    const float s = Elem<T>::ld(pred + e), t = a.target[e];
    dp[e] = s;
    dt[e] = t;
    soft += !(t == 0.0f || t == 1.0f);
    wild += !met_finite(s);
  }
  if (soft) atomicAdd(&s_bad[0], soft);
  if (wild) atomicAdd(&s_bad[1], wild);
  __syncthreads();
  if (tid < 2 && s_bad[tid]) atomicAdd(a.status + tid, s_bad[tid]);
}

// ------------------------------------------------------------------ eval (1): one block per (row tile, class)
__global__ __launch_bounds__(MET_T) void metric_tile_kernel(mds_metric_eval_args a, int N, int tiles) {
  __shared__ __attribute__((aligned(16))) float s_all[2][MET_T];      // the walked tile's scores
  __shared__ __attribute__((aligned(16))) float s_pos[2][MET_T];      // ... again where the row is positive, NaN where not
  __shared__ double s_q[MET_T];
  __shared__ int s_flag[MET_T];
  __shared__ float s_sel[MET_T];                                       // the tile's positive rows' scores, in row order
  __shared__ int s_cnt[2];
  const int tid = threadIdx.x, k = blockIdx.x, c = blockIdx.y, C = a.C;
  const float nanf_ = bits2f(0x7fc00000u);
  const int row = k * MET_T + tid;
  const bool live = row < N;
  const float sj = live ? a.pred[(long)row * C + c] : nanf_;
  const float tj = live ? a.target[(long)row * C + c] : 0.0f;
  const bool pj = live && tj == 1.0f;
  const bool hit = live && ((tj > a.threshold) == (sj > a.threshold));
  if (tid < 2) s_cnt[tid] = 0;
  __syncthreads();
  if (pj) atomicAdd(&s_cnt[0], 1);
  if (hit) atomicAdd(&s_cnt[1], 1);
  __syncthreads();
  const int npos = s_cnt[0];      // (block-uniform)
  double S = 0.0;
  if ((a.what & MDS_METRIC_AP) && npos > 0) {
    // the tile's positive rows, compacted in row order: thread r < npos takes over the score of the tile's r-th positive row, so
    // only the first ceil(npos / 64) waves compare; the other waves keep loading the walked tiles
    s_flag[tid] = pj;
    __syncthreads();
    int rank = 0;
    for (int i = 0; i < tid; ++i) rank += s_flag[i];
    if (pj) s_sel[rank] = sj;
    __syncthreads();
    const float mine = tid < npos ? s_sel[tid] : nanf_;
    const bool busy = (tid & ~(MDS_WAVE - 1)) < npos;      // (wave-uniform)
    int n = 0, tp = 0;
    // tile m of the walk lives in buffer m & 1: it is written before barrier m and read after it, and its buffer was last read
    // before barrier m - 1
    float ws = sj, wp = pj ? sj : nanf_;      // tile k first, then k + 1, ... (the counts do not depend on the order)
    for (int m = 0; m < tiles; ++m) {
      const int b = m & 1;
      s_all[b][tid] = ws;
      s_pos[b][tid] = wp;
      __syncthreads();
      if (m + 1 < tiles) {      // the next tile's loads fly during this tile's compares
        int mt = k + m + 1;
        mt = mt >= tiles ? mt - tiles : mt;
        const int r = mt * MET_T + tid;
        ws = nanf_; wp = nanf_;
        if (r < N) {
          ws = a.pred[(long)r * C + c];
          wp = a.target[(long)r * C + c] == 1.0f ? ws : nanf_;
        }
      }
      if (busy) {
#pragma unroll 4
        for (int i = 0; i < MET_T; i += 4) {
          const f32x4 va = *(const f32x4*)&s_all[b][i], vp = *(const f32x4*)&s_pos[b][i];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            n += va[u] >= mine;
            tp += vp[u] >= mine;
          }
        }
      }
    }
    s_q[tid] = tid < npos ? (double)tp / (double)n : 0.0;
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < npos; ++i) S = S + s_q[i];
  }
  if (tid == 0) {
    const MetWs w = met_ws(a.workspace, tiles, C, c);
    w.S[k] = S;
    w.pos[k] = npos;
    w.hit[k] = s_cnt[1];
  }
}

// ------------------------------------------------------------------ eval (2): one block per class adds the tiles in tile order
__global__ __launch_bounds__(256) void metric_finish_kernel(mds_metric_eval_args a, int N, int tiles) {
  __shared__ int s_cnt[2];
  const int tid = threadIdx.x, c = blockIdx.x, C = a.C;
  const MetWs w = met_ws(a.workspace, tiles, C, c);
  if (tid < 2) s_cnt[tid] = 0;
  __syncthreads();
  int p = 0, h = 0;
  for (int k = tid; k < tiles; k += 256) { p += w.pos[k]; h += w.hit[k]; }
  if (p) atomicAdd(&s_cnt[0], p);
  if (h) atomicAdd(&s_cnt[1], h);
  __syncthreads();
  if (tid != 0) return;
  if (a.what & MDS_METRIC_AP) {
    const int P = s_cnt[0];
    double total = 0.0;
    for (int k = 0; k < tiles; ++k) total = total + w.S[k];
    a.result[c] = P ? total / (double)P : 0.0;
    a.result[2L * C + c] = (double)P;
  }
  if (a.what & MDS_METRIC_ACC) a.result[(long)C + c] = (double)s_cnt[1] / (double)N;
  if (c == 0) {
    a.result[3L * C] = (double)a.status[0];
    a.result[3L * C + 1] = (double)a.status[1];
  }
}

extern "C" long mds_metric_push(const mds_metric_push_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a, "metric_push: null arguments");
  MDS_REQUIRE(a->dtype == MDS_F32 || a->dtype == MDS_BF16, "metric_push: dtype %d", a->dtype);
  MDS_REQUIRE(a->B >= 1 && a->C >= 1 && (long)a->B * a->C < 2147483647L, "metric_push: B x C = %d x %d", a->B, a->C);
  MDS_REQUIRE(a->row >= 0 && a->row + a->B <= a->capacity, "metric_push: rows %ld .. %ld of a buffer of %ld", a->row, a->row + a->B - 1, a->capacity);
  MDS_REQUIRE(a->pred && a->target && a->dst_pred && a->dst_target && a->status, "metric_push: null pred, target, epoch buffer or status");
  const long n = (long)a->B * a->C;
  const unsigned blocks = (unsigned)(n + 255) / 256 > 1024u ? 1024u : (unsigned)((n + 255) / 256);
  if (a->dtype == MDS_BF16) MDS_LAUNCH(metric_push_kernel<bf16_t>, dim3(blocks), dim3(256), 0, stream, *a);
  else MDS_LAUNCH(metric_push_kernel<float>, dim3(blocks), dim3(256), 0, stream, *a);
  return mds_check_launch("metric_push");
}

extern "C" long mds_metric_eval(const mds_metric_eval_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a, "metric_eval: null arguments");
  MDS_REQUIRE(a->N >= 1 && a->N < 2147483647L && a->C >= 1 && a->N * a->C < 2147483647L, "metric_eval: N x C = %ld x %d", a->N, a->C);
  MDS_REQUIRE(a->what >= 1 && a->what <= (MDS_METRIC_AP | MDS_METRIC_ACC), "metric_eval: what = %d", a->what);
  MDS_REQUIRE(a->pred && a->target && a->status && a->result && a->workspace, "metric_eval: null pred, target, status, result or workspace");
  MDS_REQUIRE(((uintptr_t)a->workspace & 7) == 0 && a->workspace_bytes >= MDS_METRIC_WORKSPACE_BYTES(a->N, a->C),
              "metric_eval: workspace of %ld bytes, the launch needs %ld (8-byte aligned)", a->workspace_bytes, MDS_METRIC_WORKSPACE_BYTES(a->N, a->C));
  const int N = (int)a->N, tiles = (int)MDS_METRIC_TILES(a->N);
  MDS_LAUNCH(metric_tile_kernel, dim3((unsigned)tiles, (unsigned)a->C), dim3(MET_T), 0, stream, *a, N, tiles);
  MDS_LAUNCH(metric_finish_kernel, dim3((unsigned)a->C), dim3(256), 0, stream, *a, N, tiles);
  return mds_check_launch("metric_eval");
}
