// k_spot.hip — spotting on the device (mds_spot, include/mds.h; reference src/utils.py::post_processing and
// scripts/ball_action/ensemble.py::load_and_blend_predictions): blend K prediction tracks, smooth every class's series with
// the caller's kernel, find the local maxima, select by height and distance, write the kept peaks of every class in row
// order.  Two kernels on the caller's stream, nothing returns to the host in between.
//
// The workload is small (a half: 67,500 rows x <= 15 classes; 14 tracks = 57 MB read once): the point is the missing round
// trip, not occupancy.  Kernel 1 is a streaming pass with an r-row halo in LDS (18 KB per block); kernel 2 is one block per
// class working on class-major rows of the workspace.  No floating-point atomics anywhere: the output is a pure function of
// the input.
#include "platform.h"

// the header's arithmetic contract: every product and every sum is rounded on its own (no fused multiply-add)
#pragma clang fp contract(off)

#define SPOT_T MDS_SPOT_THREADS
#define SPOT_HALO_ROWS (MDS_SPOT_TILE + 2 * MDS_SPOT_MAX_RADIUS)

// the workspace: y[C][N] doubles, then per class N candidate rows, N states, N round flags (int32)
struct SpotWs { double* y; int* cand; int* state; int* win; };
MDS_DEV SpotWs spot_ws(void* base, int N, int C, int c) {
  const long NC = (long)N * C;
  SpotWs w;
  w.y = (double*)base + (long)c * N;
  int* ib = (int*)((double*)base + NC);
  w.cand = ib + (long)c * N;
  w.state = ib + NC + (long)c * N;
  w.win = ib + 2 * NC + (long)c * N;
  return w;
}

// R of the header: d c b a | a b c d | d c b a, any i
MDS_DEV int spot_reflect(long i, int N) {
  const long P = 2L * N;
  long m = i % P;
  if (m < 0) m += P;
  return (int)(m < N ? m : P - 1 - m);
}

// x[i] of class c: the blend of the tracks that cover frame lo + i (the track index is a compile-time constant of the unrolled
// loop: the pointers are read straight from the kernel arguments)
MDS_DEV double spot_x(const mds_spot_args& a, long lo, int i, int c) {
  if (a.mode == MDS_SPOT_SINGLE) return (double)((const float*)a.track[0])[(long)i * a.C + c];
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < MDS_SPOT_MAX_TRACKS; ++k) {
    if (k < a.K) {
      const long q = lo + i - a.first[k];
      if (q >= 0 && q < a.rows[k])
        s = s + (a.track_f64 ? ((const double*)a.track[k])[q * a.C + c] : (double)((const float*)a.track[k])[q * a.C + c]);
    }
  }
  return s / (double)a.K;
}

// grid = (row tiles, class chunks).  The tile's rows [t0, t0 + rows) need x at [t0 - r, t0 + rows + r), reflected into [0, N).
__global__ __launch_bounds__(SPOT_T) void spot_smooth_kernel(mds_spot_args a, long lo, int N) {
  __shared__ double xs[SPOT_HALO_ROWS * MDS_SPOT_CLASSES];
  __shared__ double wt[2 * MDS_SPOT_MAX_RADIUS + 1];
  const int tid = threadIdx.x, r = a.radius, C = a.C;
  const int t0 = blockIdx.x * MDS_SPOT_TILE, c0 = blockIdx.y * MDS_SPOT_CLASSES;
  const int rows = N - t0 < MDS_SPOT_TILE ? N - t0 : MDS_SPOT_TILE;
  const int cc = C - c0 < MDS_SPOT_CLASSES ? C - c0 : MDS_SPOT_CLASSES;
  for (int i = tid; i < 2 * r + 1; i += SPOT_T) wt[i] = a.weights[i];
  for (int e = tid; e < (rows + 2 * r) * cc; e += SPOT_T) {
    const int h = e / cc, c = e - h * cc;
    xs[e] = spot_x(a, lo, spot_reflect((long)t0 - r + h, N), c0 + c);
  }
  __syncthreads();
  for (int e = tid; e < rows * cc; e += SPOT_T) {
    const int l = e / cc, c = e - l * cc;
    const double* x = xs + (l + r) * cc + c;
    double acc = x[0] * wt[r];
    for (int j = r; j >= 1; --j) acc = acc + (x[-j * cc] + x[j * cc]) * wt[r - j];
    const long row = t0 + l;
    double y = acc;
    if (a.mode == MDS_SPOT_SINGLE) {
      const float yf = (float)acc;
      y = (double)yf;
      if (a.smoothed) ((float*)a.smoothed)[row * C + c0 + c] = yf;
    } else if (a.smoothed) {
      ((double*)a.smoothed)[row * C + c0 + c] = acc;
    }
    ((double*)a.workspace)[(long)(c0 + c) * N + row] = y;
  }
}

// the peak whose plateau STARTS at row i (1 <= i <= N - 2): its row, or -1
MDS_DEV int spot_peak_from(const double* y, int N, int i) {
  const double v = y[i];
  if (!(y[i - 1] < v)) return -1;
  int j = i + 1;
  while (j < N - 1 && y[j] == v) ++j;
  return y[j] < v ? (i + j - 1) / 2 : -1;
}

// exclusive prefix of one int per thread over the block; *total = the sum.  s: SPOT_T ints of LDS
MDS_DEV int spot_scan(int* s, int v, int* total) {
  const int tid = threadIdx.x;
  __syncthreads();      // (s may still be read from the previous scan)
  s[tid] = v;
  __syncthreads();
  int before = 0, all = 0;
  for (int t = 0; t < SPOT_T; ++t) {
    const int n = s[t];
    before += t < tid ? n : 0;
    all += n;
  }
  *total = all;
  return before;
}

// one block per class
__global__ __launch_bounds__(SPOT_T) void spot_select_kernel(mds_spot_args a, int N) {
  __shared__ int s_n[SPOT_T];
  __shared__ int s_any;
  const int tid = threadIdx.x, c = blockIdx.x, dist = a.distance;
  const SpotWs w = spot_ws(a.workspace, N, a.C, c);
  const double* y = w.y;

  // ---- candidates: peaks that pass `height`, in row order.  A thread owns the plateau starts of its chunk of rows.
  const int L = (N + SPOT_T - 1) / SPOT_T;
  const int i0 = tid * L < 1 ? 1 : tid * L;
  const int i1 = (tid + 1) * L < N - 1 ? (tid + 1) * L : N - 1;
  int mine = 0;
  for (int i = i0; i < i1; ++i) {
    const int p = spot_peak_from(y, N, i);
    if (p >= 0 && a.height <= y[p]) ++mine;
  }
  int M;
  int at = spot_scan(s_n, mine, &M);
  for (int i = i0; i < i1; ++i) {
    const int p = spot_peak_from(y, N, i);
    if (p >= 0 && a.height <= y[p]) { w.cand[at] = p; w.state[at] = 0; ++at; }
  }

  // ---- distance: rounds of (decide, apply).  state: 0 undecided, 1 kept, 2 removed.  The undecided candidate of the highest
  // priority always wins its round, so every round decides at least one candidate.
  for (;;) {
    __syncthreads();      // the candidate list / the states of the last round's apply phase
    if (tid == 0) s_any = 0;
    __syncthreads();
    int undecided = 0;
    for (int i = tid; i < M; i += SPOT_T) {
      if (w.state[i] != 0) continue;
      undecided = 1;
      const int p = w.cand[i];
      const double v = y[p];
      int wins = 1;
      for (int k = i - 1; wins && k >= 0 && p - w.cand[k] < dist; --k)
        if (w.state[k] == 0 && y[w.cand[k]] >= v) wins = 0;      // an equal value at a lower row has priority
      for (int k = i + 1; wins && k < M && w.cand[k] - p < dist; ++k)
        if (w.state[k] == 0 && y[w.cand[k]] > v) wins = 0;
      w.win[i] = wins;
    }
    if (undecided) atomicAdd(&s_any, 1);
    __syncthreads();
    if (s_any == 0) break;      // (block-uniform)
    // two winners are never closer than `distance` (one would outrank the other), and no kept candidate of an earlier round is
    // (it would have removed this one): a winner's state is written by its own thread only, every other state written here
    // belongs to an undecided loser or to an already removed candidate, and a thread reads no state but its own candidates'
    // (a loser's may change to 2 under the read: it is skipped either way; win[] of a decided candidate is never looked at)
    for (int i = tid; i < M; i += SPOT_T) {
      if (w.state[i] != 0 || !w.win[i]) continue;
      const int p = w.cand[i];
      w.state[i] = 1;
      for (int k = i - 1; k >= 0 && p - w.cand[k] < dist; --k) w.state[k] = 2;
      for (int k = i + 1; k < M && w.cand[k] - p < dist; ++k) w.state[k] = 2;
    }
  }

  // ---- the kept peaks in row order
  const int LM = (M + SPOT_T - 1) / SPOT_T;
  const int k0 = tid * LM < M ? tid * LM : M, k1 = (tid + 1) * LM < M ? (tid + 1) * LM : M;
  int kept = 0;
  for (int k = k0; k < k1; ++k) kept += w.state[k] == 1;
  int total;
  int pos = spot_scan(s_n, kept, &total);
  for (int k = k0; k < k1; ++k) {
    if (w.state[k] != 1) continue;
    if (pos < a.cap) {
      const int p = w.cand[k];
      a.peak_index[(long)c * a.cap + pos] = p;
      a.peak_conf[(long)c * a.cap + pos] = y[p];
    }
    ++pos;
  }
  if (tid == 0) a.peak_count[c] = total;
}

extern "C" long mds_spot(const mds_spot_args* a, mds_stream_t stream) {
  MDS_REQUIRE(a, "spot: null arguments");
  MDS_REQUIRE(a->C >= 1, "spot: C = %d", a->C);
  MDS_REQUIRE(a->K >= 1 && a->K <= MDS_SPOT_MAX_TRACKS, "spot: K = %d tracks (1 .. %d)", a->K, MDS_SPOT_MAX_TRACKS);
  MDS_REQUIRE(a->mode == MDS_SPOT_SINGLE || a->mode == MDS_SPOT_BLEND, "spot: mode %d", a->mode);
  MDS_REQUIRE(a->mode != MDS_SPOT_SINGLE || (a->K == 1 && !a->track_f64), "spot: MDS_SPOT_SINGLE takes one fp32 track (K = %d)", a->K);
  MDS_REQUIRE(a->radius >= 0 && a->radius <= MDS_SPOT_MAX_RADIUS, "spot: radius = %d (0 .. %d)", a->radius, MDS_SPOT_MAX_RADIUS);
  MDS_REQUIRE(a->distance >= 1, "spot: distance = %d (>= 1)", a->distance);
  MDS_REQUIRE(a->cap >= 1, "spot: cap = %d (>= 1)", a->cap);
  MDS_REQUIRE(a->weights && a->peak_index && a->peak_conf && a->peak_count && a->workspace, "spot: null weights, peak buffer or workspace");
  // the union of the tracks' ranges, walked in the order of their first frames
  int order[MDS_SPOT_MAX_TRACKS];
  for (int k = 0; k < a->K; ++k) {
    MDS_REQUIRE(a->track[k], "spot: track %d is null", k);
    MDS_REQUIRE(a->rows[k] >= 1 && a->rows[k] < 2147483647L, "spot: track %d has %ld rows (N >= 1)", k, a->rows[k]);
    int j = k;
    for (; j > 0 && a->first[order[j - 1]] > a->first[k]; --j) order[j] = order[j - 1];
    order[j] = k;
  }
  const long lo = a->first[order[0]];
  long end = lo + a->rows[order[0]];
  for (int j = 1; j < a->K; ++j) {
    const int k = order[j];
    MDS_REQUIRE(a->first[k] <= end, "spot: no track covers frames %ld .. %ld (the union of the tracks must be contiguous)", end, a->first[k] - 1);
    const long e = a->first[k] + a->rows[k];
    end = e > end ? e : end;
  }
  const long N = end - lo;
  MDS_REQUIRE(N * a->C < 2147483647L, "spot: N x C = %ld x %d", N, a->C);
  MDS_REQUIRE(((uintptr_t)a->workspace & 7) == 0 && a->workspace_bytes >= MDS_SPOT_WORKSPACE_BYTES(N, a->C),
              "spot: workspace of %ld bytes, the launch needs %ld (8-byte aligned)", a->workspace_bytes, MDS_SPOT_WORKSPACE_BYTES(N, a->C));
  MDS_LAUNCH(spot_smooth_kernel, dim3((unsigned)cdiv(N, MDS_SPOT_TILE), (unsigned)cdiv(a->C, MDS_SPOT_CLASSES)), dim3(SPOT_T), 0, stream, *a, lo, (int)N);
  MDS_LAUNCH(spot_select_kernel, dim3((unsigned)a->C), dim3(SPOT_T), 0, stream, *a, (int)N);
  return mds_check_launch("spot");
}
