// Integrated loudness on the device (FlowHighSR.generate*(loudness=L), FlowHighSR.measure_loudness): ITU-R BS.1770-4 as
// flowhigh_amd/loudness.py defines it.
//   fh_kweight_energy_f32       float32 rows [rows, len] -> double [rows, n_sub]: the energies of the 100 ms sub-blocks of the
//                               K-weighted rows
//   fh_kweight_energy_seg_f32   the same over a device table of clips read where they are (pointer + row pitch)
//   fh_loudness_gate_f32        the sub-energies of every clip's rows -> its gated loudness and the gain to a target
//   fh_stream_kweight_energy_f32   the same over a stream that arrives in blocks: the recursion's state and the running sub-block
//                               sum start from a record in memory and are stored back to it
//   fh_loudness_report_f32      the sub-energies of every clip's rows -> EBU R128's figures (flowhigh_amd/meter.py): integrated,
//                               momentary and short-term maximum, loudness range, the last momentary and short-term value
// The three energy entries are instantiations of one kernel body that differ in the row locator (where a row's samples lie,
// where it starts and what it leaves behind), so a row gets the same bits from each.  Everything behind the float32 load is
// float64: in float32 the high-pass (poles at radius 0.995) loses up to 5e-4 of a sub-block's energy on low-frequency-heavy input.
//
// K-weighting is two biquads in cascade, a 4-state linear recurrence s' = A s + B x in transposed direct form II.  It is run in
// parallel along time and exactly (no warm-up approximation: the impulse response needs more than 4000 samples to fall to 1e-9):
//   * one workgroup owns a row and walks its spans of SPAN = 256 * CHUNK samples in order, carrying the state; span boundaries
//     are counted from the row's sample 0, so a row's result depends on the row alone;
//   * a span is staged into LDS (chunk pitch CHUNK + 1 floats: lanes reading lane * CHUNK + n do not share a bank), the next
//     span's loads already under way;
//   * every lane runs its chunk from zero state (lane 0 from the carried state) and keeps the end state z;
//   * the end states are scanned over the 256 lanes in 8 steps, e[t] += A^(CHUNK 2^i) e[t - 2^i], with the constant hand-over
//     matrices the host made in float64; e[t - 1] is then lane t's true start state and e[255] the next span's carry;
//   * every lane runs its chunk again from its true start state and adds y^2 to the sub-block of each sample: a chunk straddles
//     at most one sub-block boundary (hop >= CHUNK), so a lane has two partial sums;
//   * the lanes' partial sums of every sub-block the span touches are added in a fixed tree (wave butterfly, then the 4 waves in
//     order) and thread 0 adds the span's share to the sub-block's running sum.  Lanes outside a sub-block add an exact 0.0, so a
//     sub-block's sum does not depend on what follows it in the row.
#include <math.h>

#include "fh_common.h"

namespace {

constexpr int CHUNK = 16;                       // samples per lane and span
constexpr int THREADS = 256;
constexpr int SPAN = THREADS * CHUNK;           // 4096 samples
constexpr int PITCH = CHUNK + 1;
constexpr int SCAN_STEPS = 8;                   // log2(THREADS)
constexpr int MAX_SUB_PER_SPAN = SPAN / CHUNK + 2;
constexpr int MAX_LEN = 1 << 30;
constexpr double ZA = 0x1.f791ec6e1d5b7p-24;    // 10^((-70 + 0.691) / 10): loudness.ZA, bit for bit
constexpr double REL_GATE = 0.1;

struct kw_filter {
  double b0, b1, b2, a1, a2;                    // the shelf
  double d0, d1, d2, c1, c2;                    // the high-pass
  double M[SCAN_STEPS][16];                     // A^(CHUNK 2^i), row-major
};

struct kw_state {
  double s1, s2, t1, t2;
};

// One row as the kernel body sees it: `len` samples to walk from load(0) on, sample n lying `off() + n` samples behind the start
// of the sub-block that e()[0] holds; holds(k): whether e()[k] may be written.  start / finish: what the row begins with and
// what it leaves behind (a whole row begins at rest and leaves nothing).
struct kw_row {
  const float* x;
  int len;
  double* e_;
  __device__ bool skip() const { return len < 1; }
  __device__ float load(int n) const { return x[n]; }
  __device__ int off() const { return 0; }
  __device__ double* e() const { return e_; }
  __device__ bool holds(int) const { return true; }
  __device__ void start(kw_state&, double&, int&) const {}
  __device__ void finish(int, const kw_state&, double) const {}
};

struct BatchedRows {
  const float* x;
  int len;
  double* out;
  int out_pitch;
  __device__ kw_row operator()(int r) const { return {x + (size_t)r * len, len, out + (size_t)r * out_pitch}; }
};
struct ClipRows {                               // row r is channel (r - first row of its clip) of clip group[r] of the table
  const fh_pcm_clip* clips;
  const int32_t* group;
  int n_clips, max_len;
  double* out;
  int out_pitch;
  __device__ kw_row operator()(int r) const {
    const int g = group[r];
    if (g < 0 || g >= n_clips) return {nullptr, 0, nullptr};        // (the tables live on the device: checked)
    int ch = 0;
    while (ch < r && group[r - ch - 1] == g) ++ch;
    const fh_pcm_clip c = clips[g];
    if (ch >= c.channels || c.len < 1 || c.len > max_len || !c.src) return {nullptr, 0, nullptr};      // (its row of `out` has max_len's sub-blocks)
    return {c.src + (long long)ch * c.pitch, c.len, out + (size_t)r * out_pitch};
  }
};

// A row of a stream (fh_meter_job): the source is the kept samples, then the fresh ones, its first sample at the absolute index
// base = k0 hop + off.  The walk is the whole spans of the source (ended: all of it); the sub-block in progress at `base` is
// e()[0], its sum so far in the record.
constexpr int MAX_SUB = 1 << 20;
constexpr int MAX_FRESH = MAX_LEN - 2 * SPAN;
__host__ __device__ inline bool meter_job_ok(const fh_meter_job& j) {
  if (j.n_kept < 0 || j.n_kept >= SPAN || j.n_fresh < 0 || j.n_fresh > MAX_FRESH) return false;
  if (j.base < 0 || j.base % SPAN != 0 || j.log_len < 0 || j.log_len > MAX_SUB) return false;
  if (!j.state || !j.log || (j.n_kept > 0 && !j.kept) || (j.n_fresh > 0 && !j.fresh)) return false;
  return j.ended || (j.n_kept + j.n_fresh) % SPAN == 0 || j.keep;
}
struct kw_stream_row {
  fh_meter_job j;
  int len, off_, cap;                           // cap: the entries of the log from e() on
  bool ok;
  __device__ bool skip() const { return !ok; }
  __device__ float load(int n) const { return n < j.n_kept ? j.kept[n] : j.fresh[n - j.n_kept]; }
  __device__ int off() const { return off_; }
  __device__ double* e() const { return j.log + (j.log_len - cap); }
  __device__ bool holds(int k) const { return k < cap; }
  __device__ void start(kw_state& s, double& acc, int& acc_k) const {
    const fh_meter_state r = *j.state;
    s = {r.s1, r.s2, r.t1, r.t2};
    if (off_ > 0) {                             // (off 0: the sub-block before `base` is complete and in the log already)
      acc = r.acc;
      acc_k = 0;
    }
  }
  __device__ void finish(int t, const kw_state& s, double acc) const {
    if (t == 0) *j.state = {s.s1, s.s2, s.t1, s.t2, acc};
    for (int i = len + t; i < j.n_kept + j.n_fresh; i += THREADS) j.keep[i - len] = load(i);
  }
};
struct StreamRows {
  const fh_meter_job* jobs;
  int hop;
  __device__ kw_stream_row operator()(int r) const {
    kw_stream_row row;
    row.j = jobs[r];
    row.ok = meter_job_ok(row.j);
    row.len = row.off_ = row.cap = 0;
    if (!row.ok) return row;
    const long long k0 = row.j.base / hop;
    const int n = row.j.n_kept + row.j.n_fresh;
    row.len = row.j.ended ? n : n / SPAN * SPAN;
    row.off_ = (int)(row.j.base - k0 * hop);
    row.cap = k0 < row.j.log_len ? row.j.log_len - (int)k0 : 0;
    return row;
  }
};

__device__ __forceinline__ double kw_step(const kw_filter& f, kw_state& s, double x) {
  const double y1 = fma(f.b0, x, s.s1);
  s.s1 = fma(f.b1, x, fma(-f.a1, y1, s.s2));
  s.s2 = fma(f.b2, x, -f.a2 * y1);
  const double y = fma(f.d0, y1, s.t1);
  s.t1 = fma(f.d1, y1, fma(-f.c1, y, s.t2));
  s.t2 = fma(f.d2, y1, -f.c2 * y);
  return y;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <class Loc>
__global__ __launch_bounds__(THREADS) void kweight_energy_kernel(Loc loc, kw_filter f, int hop) {
  __shared__ float xs[THREADS * PITCH];
  __shared__ double st[2][4][THREADS];          // the scan's two buffers, component-major: lanes read consecutive doubles
  __shared__ double wpart[MAX_SUB_PER_SPAN][THREADS / 64];
  __shared__ double Ms[SCAN_STEPS * 16];        // the hand-over matrices: 128 constants are too many to hold in scalar registers
  const auto row = loc(blockIdx.x);
  if (row.skip()) return;
  const int t = threadIdx.x, T = row.len, off = row.off();
  if (t < SCAN_STEPS * 16) Ms[t] = f.M[t / 16][t % 16];             // (the first span's barriers come before its first read)
  double* __restrict__ e = row.e();

  kw_state carry = {0.0, 0.0, 0.0, 0.0};
  double acc = 0.0;                             // (thread 0) the running sum of sub-block acc_k
  int acc_k = -1;
  row.start(carry, acc, acc_k);
  float xn[CHUNK];                              // the next span's samples, loaded while this one is worked on
#pragma unroll
  for (int k = 0; k < CHUNK; ++k) {
    const int n = k * THREADS + t;
    xn[k] = n < T ? row.load(n) : 0.f;
  }
  for (int span0 = 0; span0 < T; span0 += SPAN) {
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) {
      const int idx = k * THREADS + t;
      xs[(idx / CHUNK) * PITCH + (idx % CHUNK)] = xn[k];
    }
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) {
      const int n = span0 + SPAN + k * THREADS + t;
      xn[k] = n < T ? row.load(n) : 0.f;
    }
    __syncthreads();
    float xr[CHUNK];
#pragma unroll
    for (int n = 0; n < CHUNK; ++n) xr[n] = xs[t * PITCH + n];

    // the chunk from zero state (lane 0: from the carried state, its true start)
    kw_state s = {0.0, 0.0, 0.0, 0.0};
    if (t == 0) s = carry;
#pragma unroll
    for (int n = 0; n < CHUNK; ++n) kw_step(f, s, (double)xr[n]);

    // inclusive scan of e[t] = A^CHUNK e[t - 1] + z[t]
    double v[4] = {s.s1, s.s2, s.t1, s.t2};
    int cur = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) st[0][c][t] = v[c];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SCAN_STEPS; ++i) {
      const int d = 1 << i;
      if (t >= d) {
        double u[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) u[c] = st[cur][c][t - d];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double a = v[r];
#pragma unroll
          for (int c = 0; c < 4; ++c) a = fma(Ms[16 * i + 4 * r + c], u[c], a);
          v[r] = a;
        }
      }
      cur ^= 1;
#pragma unroll
      for (int c = 0; c < 4; ++c) st[cur][c][t] = v[c];
      __syncthreads();
    }
    s = carry;
    if (t > 0) s = {st[cur][0][t - 1], st[cur][1][t - 1], st[cur][2][t - 1], st[cur][3][t - 1]};
    carry = {st[cur][0][THREADS - 1], st[cur][1][THREADS - 1], st[cur][2][THREADS - 1], st[cur][3][THREADS - 1]};

    // the chunk again from its true start state: y^2 into the (at most two) sub-blocks of its samples
    const int n0 = span0 + t * CHUNK;
    const int k0 = (off + n0) / hop;
    const int edge = (k0 + 1) * hop - (off + n0);                   // samples of the chunk in sub-block k0 (or more than CHUNK)
    double p0 = 0.0, p1 = 0.0;
#pragma unroll
    for (int n = 0; n < CHUNK; ++n) {
      const double y = kw_step(f, s, (double)xr[n]);
      const double sq = (n0 + n < T) ? y * y : 0.0;
      p0 += n < edge ? sq : 0.0;
      p1 += n < edge ? 0.0 : sq;
    }
    const int span_end = min(T, span0 + SPAN);
    const int k_first = (off + span0) / hop, nk = (off + span_end - 1) / hop - k_first + 1;
    for (int kk = 0; kk < nk; ++kk) {
      const int k = k_first + kk;
      const double w = wave_sum_f64(k == k0 ? p0 : (k == k0 + 1 ? p1 : 0.0));
      if ((t & 63) == 0) wpart[kk][t >> 6] = w;
    }
    __syncthreads();
    if (t == 0) {
      for (int kk = 0; kk < nk; ++kk) {
        const double total = ((wpart[kk][0] + wpart[kk][1]) + wpart[kk][2]) + wpart[kk][3];
        const int k = k_first + kk;
        if (k == acc_k) {
          acc += total;
        } else {
          if (acc_k >= 0 && row.holds(acc_k)) e[acc_k] = acc;
          acc_k = k;
          acc = total;
        }
      }
    }
  }
  if (t == 0 && acc_k >= 0 && row.holds(acc_k)) e[acc_k] = acc;
  row.finish(t, carry, acc);
}

// ---- a clip's energies -> its figures: one workgroup per clip, its rows those r with group[r] == clip ------------------------------
struct clip_view {
  const double* e0;                             // the clip's first row of the energies
  int C, r0, T, n_sub, nb;                      // rows, first row, samples, sub-blocks, 400 ms blocks (0: nothing to read)
  bool is_short;
};

// (all threads; two barriers)
__device__ __forceinline__ clip_view find_clip(const double* __restrict__ e, int e_pitch, const int32_t* __restrict__ lens,
                                               const int32_t* __restrict__ group, int rows, int hop, int clip, int* first_row,
                                               int* n_rows) {
  const int t = threadIdx.x;
  if (t == 0) {
    *first_row = rows;
    *n_rows = 0;
  }
  __syncthreads();
  for (int r = t; r < rows; r += THREADS)
    if (group[r] == clip) {
      atomicMin(first_row, r);
      atomicAdd(n_rows, 1);
    }
  __syncthreads();
  clip_view v;
  v.r0 = *first_row, v.C = *n_rows;
  v.e0 = nullptr, v.T = v.n_sub = v.nb = 0, v.is_short = false;
  if (v.C == 0) return v;
  const int T = lens[v.r0], block = 4 * hop;
  v.T = T;
  v.n_sub = T > 0 ? (T + hop - 1) / hop : 0;
  v.is_short = T < block;
  // (lens lives on the device: a row longer than its row of `e` holds is not read, the clip measures as silent)
  v.nb = (T < 1 || v.n_sub > e_pitch) ? 0 : (v.is_short ? 1 : (T - block) / hop + 1);
  v.e0 = e + (size_t)v.r0 * e_pitch;
  return v;
}

// z[j], the energy of the clip's 400 ms block j < nb (a short clip's only block: all of it)
__device__ __forceinline__ double block_energy(const clip_view& v, int e_pitch, int hop, int j) {
  double z = 0.0;
  if (v.is_short) {
    for (int c = 0; c < v.C; ++c)
      for (int i = 0; i < v.n_sub; ++i) z += v.e0[(size_t)c * e_pitch + i];
    z /= (double)v.T;
  } else {
    for (int c = 0; c < v.C; ++c) {
      const double* p = v.e0 + (size_t)c * e_pitch + j;
      z += ((p[0] + p[1]) + p[2]) + p[3];
    }
    z /= (double)(4 * hop);
  }
  return z;
}

// The gated loudness of the clip as the float32 that is reported.  Blocks are taken 256 at a time: every thread makes one
// block energy, thread 0 adds the chunk in ascending block order.  (all threads; zc [THREADS], res [2]: LDS)
__device__ __forceinline__ float gated_loudness(const clip_view& v, int e_pitch, int hop, double* zc, double* res) {
  const int t = threadIdx.x, nb = v.nb;
  double thr = 0.0, sum = 0.0, cnt = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    sum = 0.0;
    cnt = 0.0;
    for (int j0 = 0; j0 < nb; j0 += THREADS) {
      const int j = j0 + t;
      if (j < nb) zc[t] = block_energy(v, e_pitch, hop, j);
      __syncthreads();
      if (t == 0) {
        const int m = min(THREADS, nb - j0);
        for (int i = 0; i < m; ++i) {
          const double z = zc[i];
          if (z > ZA && z > thr) {              // (both strict; a NaN passes neither)
            sum += z;
            cnt += 1.0;
          }
        }
      }
      __syncthreads();
    }
    if (t == 0) {
      res[0] = sum;
      res[1] = cnt;
    }
    __syncthreads();
    sum = res[0];
    cnt = res[1];
    __syncthreads();
    if (cnt == 0.0) break;
    thr = REL_GATE * sum / cnt;
  }
  return cnt > 0.0 ? (float)(-0.691 + 10.0 * log10(sum / cnt)) : -INFINITY;
}

__global__ __launch_bounds__(THREADS) void loudness_gate_kernel(const double* __restrict__ e, int e_pitch,
                                                                const int32_t* __restrict__ lens, const int32_t* __restrict__ group,
                                                                int rows, int hop, double target,
                                                                const uint32_t* __restrict__ peak_bits, float* __restrict__ lufs,
                                                                float* __restrict__ gains) {
  __shared__ int first_row, n_rows;
  __shared__ double zc[THREADS];
  __shared__ double res[2];
  const int t = threadIdx.x, clip = blockIdx.x;
  const clip_view v = find_clip(e, e_pitch, lens, group, rows, hop, clip, &first_row, &n_rows);
  const int r0 = v.r0, C = v.C;
  if (C == 0) {
    if (t == 0) lufs[clip] = -INFINITY;
    return;
  }
  const float L = gated_loudness(v, e_pitch, hop, zc, res);
  uint32_t pk = 0;
  for (int c = 0; c < C; ++c) pk = max(pk, peak_bits[r0 + c]);       // (non-negative float bits order as integers)
  const double peak = (double)__uint_as_float(pk);
  float g = 1.f;
  // the gain is a function of the float32 loudness that is reported, so a caller can restate it from measure_loudness
  if (isfinite(L) && isfinite(target) && isfinite(peak) && peak > 0.0)
    g = (float)fmin(pow(10.0, (target - (double)L) / 20.0), 0.99 / peak);
  if (t == 0) lufs[clip] = L;
  if (t < C) gains[r0 + t] = g;
}

// ---- the report (flowhigh_amd/meter.py) ---------------------------------------------------------------------------------------
constexpr int ST_SUB = 30;                      // sub-blocks of a short-term window (3 s)
constexpr double LRA_REL_GATE = 0.01;           // -20 LU

// Fixed-tree reductions over the workgroup, the result in every thread (red [THREADS / 64]: LDS; two barriers).
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return r;
}
__device__ __forceinline__ double block_max_f64(double v, double* red) {      // (of values >= 0; a NaN is never the larger)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
  for (int w = 1; w < THREADS / 64; ++w) r = red[w] > r ? red[w] : r;
  __syncthreads();
  return r;
}

// Every short-term window of the clip, 256 at a time: the channel sums s[j0 .. j0 + 256 + 29) go to LDS (a thread makes one or
// two), then thread t adds window j0 + t's 30 terms in ascending order and hands zs to `use`.  (all threads; sw [THREADS + ST_SUB]: LDS)
template <class Use>
__device__ __forceinline__ void sweep_windows(const clip_view& v, int e_pitch, int hop, int ns, double* sw, Use use) {
  const int t = threadIdx.x, K = ns + ST_SUB - 1;
  const double len = (double)ST_SUB * (double)hop;
  for (int j0 = 0; j0 < ns; j0 += THREADS) {
    for (int i = t; i < THREADS + ST_SUB - 1; i += THREADS) {
      double s = 0.0;
      if (j0 + i < K)
        for (int c = 0; c < v.C; ++c) s += v.e0[(size_t)c * e_pitch + j0 + i];
      sw[i] = s;
    }
    __syncthreads();
    if (j0 + t < ns) {
      double z = sw[t];
#pragma unroll
      for (int i = 1; i < ST_SUB; ++i) z += sw[t + i];
      use(j0 + t, z / len);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ float lufs_of(double z) { return (float)(-0.691 + 10.0 * log10(z)); }     // (z = 0: -inf)

__global__ __launch_bounds__(THREADS) void loudness_report_kernel(const double* __restrict__ e, int e_pitch,
                                                                  const int32_t* __restrict__ lens, const int32_t* __restrict__ group,
                                                                  int rows, int hop, float* __restrict__ report) {
  __shared__ int first_row, n_rows;
  __shared__ double zc[THREADS];
  __shared__ double res[2];
  __shared__ double red[THREADS / 64];
  __shared__ double sw[THREADS + ST_SUB];
  __shared__ int hist[2][THREADS];              // the digit counts of the two percentiles, then their inclusive scans
  __shared__ unsigned long long prefix[2];      // the digits found so far
  __shared__ int rank[2];                       // the rank looked for among the windows that share the prefix
  const int t = threadIdx.x, clip = blockIdx.x;
  float* __restrict__ out = report + 6 * (size_t)clip;
  const clip_view v = find_clip(e, e_pitch, lens, group, rows, hop, clip, &first_row, &n_rows);
  if (v.C == 0 || v.nb == 0) {
    if (t < 6) out[t] = t == 3 ? 0.f : -INFINITY;
    return;
  }
  const float I = gated_loudness(v, e_pitch, hop, zc, res);

  // momentary: the blocks of the gate once more, their maximum and the last one
  double m_max = 0.0;
  for (int j = t; j < v.nb; j += THREADS) {
    const double z = block_energy(v, e_pitch, hop, j);
    m_max = z > m_max ? z : m_max;
  }
  m_max = block_max_f64(m_max, red);
  const double m_last = block_energy(v, e_pitch, hop, v.nb - 1);

  // short-term: maximum, last, and the absolute gate's mean
  const int K = v.T / hop, ns = K >= ST_SUB ? K - ST_SUB + 1 : 0;
  double s_max = 0.0, s_last = 0.0, a_sum = 0.0, a_cnt = 0.0;
  sweep_windows(v, e_pitch, hop, ns, sw, [&](int j, double z) {
    s_max = z > s_max ? z : s_max;
    if (j == ns - 1) s_last = z;
    if (z > ZA) {
      a_sum += z;
      a_cnt += 1.0;
    }
  });
  s_max = block_max_f64(s_max, red);
  s_last = block_sum_f64(s_last, red);          // (one thread holds it, the others an exact 0)
  a_sum = block_sum_f64(a_sum, red);
  a_cnt = block_sum_f64(a_cnt, red);

  // the range: the survivors of both gates are counted, then the two percentiles are selected digit by digit from the top:
  // positive doubles order as their bit patterns
  double lra = 0.0;
  if (a_cnt > 0.0) {
    const double thr = LRA_REL_GATE * (a_sum / a_cnt);
    double n_f = 0.0;
    sweep_windows(v, e_pitch, hop, ns, sw, [&](int, double z) { n_f += (z > ZA && z > thr) ? 1.0 : 0.0; });
    const int n = (int)block_sum_f64(n_f, red);
    if (n > 0) {
      if (t == 0) {
        rank[0] = (10 * (n - 1) + 50) / 100;
        rank[1] = (int)((95LL * (n - 1) + 50) / 100);
        prefix[0] = prefix[1] = 0;
      }
      for (int shift = 56; shift >= 0; shift -= 8) {
        hist[0][t] = 0;
        hist[1][t] = 0;
        __syncthreads();
        const unsigned long long p0 = prefix[0], p1 = prefix[1];
        sweep_windows(v, e_pitch, hop, ns, sw, [&](int, double z) {
          if (z > ZA && z > thr) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(z);
            const unsigned long long hi = shift == 56 ? 0ull : b >> (shift + 8);
            const int d = (int)((b >> shift) & 255);
            if (hi == p0) atomicAdd(&hist[0][d], 1);
            if (hi == p1) atomicAdd(&hist[1][d], 1);
          }
        });
        // (the sweep's last barrier is behind the counts) inclusive scans of both histograms, 8 steps
        for (int d = 1; d < THREADS; d <<= 1) {
          const int a0 = t >= d ? hist[0][t - d] : 0, a1 = t >= d ? hist[1][t - d] : 0;
          __syncthreads();
          hist[0][t] += a0;
          hist[1][t] += a1;
          __syncthreads();
        }
        const int r0 = rank[0], r1 = rank[1];
        const int ex0 = t ? hist[0][t - 1] : 0, ex1 = t ? hist[1][t - 1] : 0;
        const int in0 = hist[0][t], in1 = hist[1][t];
        __syncthreads();
        if (ex0 <= r0 && r0 < in0) {            // (one thread: the digit whose windows hold the rank)
          prefix[0] = (p0 << 8) | (unsigned)t;
          rank[0] = r0 - ex0;
        }
        if (ex1 <= r1 && r1 < in1) {
          prefix[1] = (p1 << 8) | (unsigned)t;
          rank[1] = r1 - ex1;
        }
        __syncthreads();
      }
      const double lo = __longlong_as_double((long long)prefix[0]), hi = __longlong_as_double((long long)prefix[1]);
      lra = 10.0 * log10(hi / lo);
    }
  }
  if (t == 0) {
    out[0] = I;
    out[1] = lufs_of(m_max);
    out[2] = ns > 0 ? lufs_of(s_max) : -INFINITY;
    out[3] = (float)lra;
    out[4] = lufs_of(m_last);
    out[5] = ns > 0 ? lufs_of(s_last) : -INFINITY;
  }
}

// c: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 -> the filter and its hand-over matrices A^(CHUNK 2^i)
kw_filter make_filter(const double* c) {
  kw_filter f;
  f.b0 = c[0], f.b1 = c[1], f.b2 = c[2], f.a1 = c[3], f.a2 = c[4];
  f.d0 = c[5], f.d1 = c[6], f.d2 = c[7], f.c1 = c[8], f.c2 = c[9];
  // s' = A s (+ B x) of kw_step: y1 = s1, y = d0 s1 + t1 at x = 0
  double A[16] = {-f.a1, 1.0, 0.0, 0.0,
                  -f.a2, 0.0, 0.0, 0.0,
                  f.d1 - f.c1 * f.d0, 0.0, -f.c1, 1.0,
                  f.d2 - f.c2 * f.d0, 0.0, -f.c2, 0.0};
  auto mul = [](const double* a, const double* b, double* o) {
    double r[16];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        double s = 0.0;
        for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
        r[4 * i + j] = s;
      }
    for (int i = 0; i < 16; ++i) o[i] = r[i];
  };
  double P[16];
  for (int i = 0; i < 16; ++i) P[i] = A[i];
  for (int n = 1; n < CHUNK; n *= 2) mul(P, P, P);                  // A^CHUNK (CHUNK is a power of two)
  for (int i = 0; i < SCAN_STEPS; ++i) {
    for (int j = 0; j < 16; ++j) f.M[i][j] = P[j];
    mul(P, P, P);
  }
  return f;
}

bool finite_coef(const double* c) {
  for (int i = 0; i < 10; ++i)
    if (!std::isfinite(c[i])) return false;
  return true;
}

}  // namespace

static_assert((CHUNK & (CHUNK - 1)) == 0, "make_filter squares its way to A^CHUNK");

extern "C" int fh_loudness_span_len(void) { return SPAN; }

extern "C" int fh_kweight_energy_f32(const float* x, const double* coef, double* energies, int rows, int len, int hop,
                                     void* stream) {
  FH_CHECK_ARG(x && coef && energies, "fh_kweight_energy_f32: null pointer (x %p, coef %p, energies %p)", (const void*)x,
               (const void*)coef, (void*)energies);
  FH_CHECK_ARG(rows > 0 && rows < 65536, "fh_kweight_energy_f32: %d rows (1 .. 65535)", rows);
  FH_CHECK_ARG(len > 0 && len <= MAX_LEN, "fh_kweight_energy_f32: len %d (1 .. 2^30)", len);
  FH_CHECK_ARG(hop >= CHUNK && hop <= MAX_LEN, "fh_kweight_energy_f32: hop %d (%d .. 2^30)", hop, CHUNK);
  FH_CHECK_ARG((((size_t)x) & 3) == 0 && (((size_t)energies) & 7) == 0,
               "fh_kweight_energy_f32: x must be 4-byte, energies 8-byte aligned");
  FH_CHECK_ARG(finite_coef(coef), "fh_kweight_energy_f32: a filter coefficient is not finite");
  hipLaunchKernelGGL(kweight_energy_kernel<BatchedRows>, dim3(rows), dim3(THREADS), 0, (hipStream_t)stream,
                     BatchedRows{x, len, energies, fh_cdiv(len, hop)}, make_filter(coef), hop);
  FH_CHECK_LAUNCH("fh_kweight_energy_f32");
  return FH_OK;
}

extern "C" int fh_kweight_energy_seg_f32(const fh_pcm_clip* clips, const int32_t* group, int n_clips, int rows, int max_len,
                                         const double* coef, double* energies, int hop, void* stream) {
  FH_CHECK_ARG(clips && group && coef && energies, "fh_kweight_energy_seg_f32: null pointer (clips %p, group %p, coef %p, "
               "energies %p)", (const void*)clips, (const void*)group, (const void*)coef, (void*)energies);
  FH_CHECK_ARG(n_clips > 0 && n_clips <= rows && rows < 65536, "fh_kweight_energy_seg_f32: %d clips of %d rows (1 <= clips <= "
               "rows <= 65535)", n_clips, rows);
  FH_CHECK_ARG(max_len > 0 && max_len <= MAX_LEN, "fh_kweight_energy_seg_f32: max_len %d (1 .. 2^30)", max_len);
  FH_CHECK_ARG(hop >= CHUNK && hop <= MAX_LEN, "fh_kweight_energy_seg_f32: hop %d (%d .. 2^30)", hop, CHUNK);
  FH_CHECK_ARG((((size_t)energies) & 7) == 0, "fh_kweight_energy_seg_f32: energies must be 8-byte aligned");
  FH_CHECK_ARG(finite_coef(coef), "fh_kweight_energy_seg_f32: a filter coefficient is not finite");
  hipLaunchKernelGGL(kweight_energy_kernel<ClipRows>, dim3(rows), dim3(THREADS), 0, (hipStream_t)stream,
                     ClipRows{clips, group, n_clips, max_len, energies, fh_cdiv(max_len, hop)}, make_filter(coef), hop);
  FH_CHECK_LAUNCH("fh_kweight_energy_seg_f32");
  return FH_OK;
}

extern "C" int fh_loudness_gate_f32(const double* energies, int n_sub, const int32_t* lens, const int32_t* group, int rows,
                                    int n_clips, int hop, double target, const uint32_t* peak_bits, float* lufs, float* gains,
                                    void* stream) {
  FH_CHECK_ARG(energies && lens && group && peak_bits && lufs && gains, "fh_loudness_gate_f32: null pointer (energies %p, lens %p, "
               "group %p, peak_bits %p, lufs %p, gains %p)", (const void*)energies, (const void*)lens, (const void*)group,
               (const void*)peak_bits, (void*)lufs, (void*)gains);
  FH_CHECK_ARG(n_clips > 0 && n_clips <= rows && rows < 65536, "fh_loudness_gate_f32: %d clips of %d rows (1 <= clips <= rows "
               "<= 65535)", n_clips, rows);
  FH_CHECK_ARG(n_sub > 0 && hop >= CHUNK && hop <= MAX_LEN / 4, "fh_loudness_gate_f32: n_sub %d must be positive, hop %d at least %d",
               n_sub, hop, CHUNK);
  FH_CHECK_ARG(target != target || (target >= -70.0 && target <= 0.0), "fh_loudness_gate_f32: target %g LUFS (-70 .. 0, or NaN: "
               "measure only)", target);
  FH_CHECK_ARG((((size_t)energies) & 7) == 0, "fh_loudness_gate_f32: energies must be 8-byte aligned");
  hipLaunchKernelGGL(loudness_gate_kernel, dim3(n_clips), dim3(THREADS), 0, (hipStream_t)stream, energies, n_sub, lens, group, rows,
                     hop, target, peak_bits, lufs, gains);
  FH_CHECK_LAUNCH("fh_loudness_gate_f32");
  return FH_OK;
}

extern "C" int fh_loudness_report_f32(const double* energies, int n_sub, const int32_t* lens, const int32_t* group, int rows,
                                      int n_clips, int hop, float* report, void* stream) {
  FH_CHECK_ARG(energies && lens && group && report, "fh_loudness_report_f32: null pointer (energies %p, lens %p, group %p, "
               "report %p)", (const void*)energies, (const void*)lens, (const void*)group, (void*)report);
  FH_CHECK_ARG(n_clips > 0 && n_clips <= rows && rows < 65536, "fh_loudness_report_f32: %d clips of %d rows (1 <= clips <= rows "
               "<= 65535)", n_clips, rows);
  FH_CHECK_ARG(n_sub > 0 && n_sub <= MAX_SUB, "fh_loudness_report_f32: n_sub %d (1 .. 2^20)", n_sub);
  FH_CHECK_ARG(hop >= CHUNK && hop <= MAX_LEN / 4, "fh_loudness_report_f32: hop %d (%d .. 2^28)", hop, CHUNK);
  FH_CHECK_ARG((((size_t)energies) & 7) == 0 && (((size_t)report) & 3) == 0,
               "fh_loudness_report_f32: energies must be 8-byte, report 4-byte aligned");
  hipLaunchKernelGGL(loudness_report_kernel, dim3(n_clips), dim3(THREADS), 0, (hipStream_t)stream, energies, n_sub, lens, group,
                     rows, hop, report);
  FH_CHECK_LAUNCH("fh_loudness_report_f32");
  return FH_OK;
}

extern "C" int fh_sizeof_meter_state(void) { return (int)sizeof(fh_meter_state); }
extern "C" int fh_sizeof_meter_job(void) { return (int)sizeof(fh_meter_job); }

extern "C" int fh_stream_kweight_energy_f32(const fh_meter_job* jobs, const fh_meter_job* check, int n_jobs, const double* coef,
                                            int hop, void* stream) {
  FH_CHECK_ARG(jobs && check && coef, "fh_stream_kweight_energy_f32: null pointer (jobs %p, check %p, coef %p)", (const void*)jobs,
               (const void*)check, (const void*)coef);
  FH_CHECK_ARG(n_jobs > 0 && n_jobs < 65536, "fh_stream_kweight_energy_f32: %d jobs (1 .. 65535)", n_jobs);
  FH_CHECK_ARG(hop >= CHUNK && hop <= MAX_LEN / 4, "fh_stream_kweight_energy_f32: hop %d (%d .. 2^28)", hop, CHUNK);
  FH_CHECK_ARG(finite_coef(coef), "fh_stream_kweight_energy_f32: a filter coefficient is not finite");
  for (int i = 0; i < n_jobs; ++i) {
    const fh_meter_job& j = check[i];
    FH_CHECK_ARG(j.base >= 0 && j.base % SPAN == 0, "fh_stream_kweight_energy_f32: job %d: base %lld is not a multiple of the span "
                 "length %d", i, (long long)j.base, SPAN);
    FH_CHECK_ARG(meter_job_ok(j), "fh_stream_kweight_energy_f32: job %d: n_kept %d (0 .. %d), n_fresh %d (0 .. 2^30 - %d), log_len %d "
                 "(0 .. 2^20), or a null pointer (kept %p, fresh %p, keep %p, state %p, log %p)", i, j.n_kept, SPAN - 1, j.n_fresh,
                 2 * SPAN, j.log_len, (const void*)j.kept, (const void*)j.fresh, (void*)j.keep, (void*)j.state, (void*)j.log);
    FH_CHECK_ARG((((size_t)j.kept | (size_t)j.fresh | (size_t)j.keep) & 3) == 0 && (((size_t)j.state | (size_t)j.log) & 7) == 0,
                 "fh_stream_kweight_energy_f32: job %d: samples must be 4-byte, state and log 8-byte aligned", i);
  }
  hipLaunchKernelGGL(kweight_energy_kernel<StreamRows>, dim3(n_jobs), dim3(THREADS), 0, (hipStream_t)stream, StreamRows{jobs, hop},
                     make_filter(coef), hop);
  FH_CHECK_LAUNCH("fh_stream_kweight_energy_f32");
  return FH_OK;
}
