// Integrated loudness on the device (FlowHighSR.generate*(loudness=L), FlowHighSR.measure_loudness): ITU-R BS.1770-4 as
// flowhigh_amd/loudness.py defines it.
//   fh_kweight_energy_f32       float32 rows [rows, len] -> double [rows, n_sub]: the energies of the 100 ms sub-blocks of the
//                               K-weighted rows
//   fh_kweight_energy_seg_f32   the same over a device table of clips read where they are (pointer + row pitch)
//   fh_loudness_gate_f32        the sub-energies of every clip's rows -> its gated loudness and the gain to a target
// The two energy entries are instantiations of one kernel body that differ in the row locator, so a row gets the same bits from
// either.  Everything behind the float32 load is float64: in float32 the high-pass (poles at radius 0.995) loses up to 5e-4 of a
// sub-block's energy on low-frequency-heavy input.
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

struct kw_row {                                 // one row as the kernel body sees it
  const float* x;
  int len;
};

struct BatchedRows {
  const float* x;
  int len;
  __device__ kw_row operator()(int r) const { return {x + (size_t)r * len, len}; }
};
struct ClipRows {                               // row r is channel (r - first row of its clip) of clip group[r] of the table
  const fh_pcm_clip* clips;
  const int32_t* group;
  int n_clips, max_len;
  __device__ kw_row operator()(int r) const {
    const int g = group[r];
    if (g < 0 || g >= n_clips) return {nullptr, 0};                 // (the tables live on the device: checked)
    int ch = 0;
    while (ch < r && group[r - ch - 1] == g) ++ch;
    const fh_pcm_clip c = clips[g];
    if (ch >= c.channels || c.len < 1 || c.len > max_len || !c.src) return {nullptr, 0};      // (its row of `out` has max_len's sub-blocks)
    return {c.src + (long long)ch * c.pitch, c.len};
  }
};

struct kw_state {
  double s1, s2, t1, t2;
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
__global__ __launch_bounds__(THREADS) void kweight_energy_kernel(Loc loc, kw_filter f, double* __restrict__ out, int out_pitch,
                                                                 int hop) {
  __shared__ float xs[THREADS * PITCH];
  __shared__ double st[2][4][THREADS];          // the scan's two buffers, component-major: lanes read consecutive doubles
  __shared__ double wpart[MAX_SUB_PER_SPAN][THREADS / 64];
  __shared__ double Ms[SCAN_STEPS * 16];        // the hand-over matrices: 128 constants are too many to hold in scalar registers
  const kw_row row = loc(blockIdx.x);
  if (row.len < 1) return;
  const int t = threadIdx.x, T = row.len;
  if (t < SCAN_STEPS * 16) Ms[t] = f.M[t / 16][t % 16];             // (the first span's barriers come before its first read)
  double* __restrict__ e = out + (size_t)blockIdx.x * out_pitch;
  const float* __restrict__ x = row.x;

  kw_state carry = {0.0, 0.0, 0.0, 0.0};
  double acc = 0.0;                             // (thread 0) the running sum of sub-block acc_k
  int acc_k = -1;
  float xn[CHUNK];                              // the next span's samples, loaded while this one is worked on
#pragma unroll
  for (int k = 0; k < CHUNK; ++k) {
    const int n = k * THREADS + t;
    xn[k] = n < T ? x[n] : 0.f;
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
      xn[k] = n < T ? x[n] : 0.f;
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
    const int k0 = n0 / hop;
    const int edge = (k0 + 1) * hop - n0;       // samples of the chunk in sub-block k0 (or more than CHUNK)
    double p0 = 0.0, p1 = 0.0;
#pragma unroll
    for (int n = 0; n < CHUNK; ++n) {
      const double y = kw_step(f, s, (double)xr[n]);
      const double sq = (n0 + n < T) ? y * y : 0.0;
      p0 += n < edge ? sq : 0.0;
      p1 += n < edge ? 0.0 : sq;
    }
    const int span_end = min(T, span0 + SPAN);
    const int k_first = span0 / hop, nk = (span_end - 1) / hop - k_first + 1;
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
          if (acc_k >= 0) e[acc_k] = acc;
          acc_k = k;
          acc = total;
        }
      }
    }
  }
  if (t == 0 && acc_k >= 0) e[acc_k] = acc;
}

// One workgroup per clip: its rows are those r with group[r] == clip.  Blocks are taken 256 at a time: every thread makes one
// block energy, thread 0 adds the chunk in ascending block order.
__global__ __launch_bounds__(THREADS) void loudness_gate_kernel(const double* __restrict__ e, int e_pitch,
                                                                const int32_t* __restrict__ lens, const int32_t* __restrict__ group,
                                                                int rows, int hop, double target,
                                                                const uint32_t* __restrict__ peak_bits, float* __restrict__ lufs,
                                                                float* __restrict__ gains) {
  __shared__ int first_row, n_rows;
  __shared__ double zc[THREADS];
  __shared__ double res[2];
  const int t = threadIdx.x, clip = blockIdx.x;
  if (t == 0) {
    first_row = rows;
    n_rows = 0;
  }
  __syncthreads();
  for (int r = t; r < rows; r += THREADS)
    if (group[r] == clip) {
      atomicMin(&first_row, r);
      atomicAdd(&n_rows, 1);
    }
  __syncthreads();
  const int r0 = first_row, C = n_rows;
  if (C == 0) {
    if (t == 0) lufs[clip] = -INFINITY;
    return;
  }
  const int T = lens[r0], block = 4 * hop;
  const int n_sub = T > 0 ? (T + hop - 1) / hop : 0;
  const bool is_short = T < block;
  // (lens lives on the device: a row longer than its row of `e` holds is not read, the clip measures as silent)
  const int nb = (T < 1 || n_sub > e_pitch) ? 0 : (is_short ? 1 : (T - block) / hop + 1);
  const double* __restrict__ e0 = e + (size_t)r0 * e_pitch;

  double thr = 0.0, sum = 0.0, cnt = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    sum = 0.0;
    cnt = 0.0;
    for (int j0 = 0; j0 < nb; j0 += THREADS) {
      const int j = j0 + t;
      if (j < nb) {
        double z = 0.0;
        if (is_short) {
          for (int c = 0; c < C; ++c)
            for (int i = 0; i < n_sub; ++i) z += e0[(size_t)c * e_pitch + i];
          z /= (double)T;
        } else {
          for (int c = 0; c < C; ++c) {
            const double* p = e0 + (size_t)c * e_pitch + j;
            z += ((p[0] + p[1]) + p[2]) + p[3];
          }
          z /= (double)block;
        }
        zc[t] = z;
      }
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
  const float L = cnt > 0.0 ? (float)(-0.691 + 10.0 * log10(sum / cnt)) : -INFINITY;
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
  hipLaunchKernelGGL(kweight_energy_kernel<BatchedRows>, dim3(rows), dim3(THREADS), 0, (hipStream_t)stream, BatchedRows{x, len},
                     make_filter(coef), energies, fh_cdiv(len, hop), hop);
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
                     ClipRows{clips, group, n_clips, max_len}, make_filter(coef), energies, fh_cdiv(max_len, hop), hop);
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
