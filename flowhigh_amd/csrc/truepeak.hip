// True peak and the look-ahead limiter on the device (FlowHighSR.generate*(true_peak=, limiter=), FlowHighSR.measure_true_peak):
// ITU-R BS.1770-4 Annex 2 as flowhigh_amd/truepeak.py defines it.
//   fh_true_peak_f32 / _seg_f32      float32 rows -> the 4x oversampled peak of every row, as non-negative float bits
//   fh_tp_envelope_f32 / _seg_f32    clips -> m[n], the oversampled envelope over the clip's channels
//   fh_limit_f32 / _seg_f32          clips and their envelopes -> the limited clips (in place or to a destination)
//   fh_delivery_gain_f32             the per-row gain of a delivery from the clip's loudness, sample peak and true peak
// The batched and segment entries of a pair are instantiations of one kernel body that differ in the locator, so a clip gets the
// same bits from either; tiles are counted from a clip's sample 0, so a clip's result depends on the clip alone.
//
// Oversampling (tp_tile): a workgroup owns TILE frames of one row, staged with HALO samples either side into LDS (zero outside
// the row).  Lane t takes frames t, t + 256, ...: its reads xs[i + 20 - k] are consecutive over the lanes (no bank conflict), the
// taps are LDS broadcasts.  The four phases (21 / 20 / 20 / 20 taps) are float32 FMA chains in ascending tap order.
//
// Limiter (limit_kernel): grid (tile, clip), TILE frames each.  r over the tile +- 2 H goes to LDS (1 outside the clip), the
// sliding minimum over 2 H + 1 is made by doubling (a[j] = min r[j .. j + P), P the largest power of two <= 2 H + 1, then two
// overlapping windows), the Hann FIR runs in float64 in ascending k from the host's double table (gain_tile), and the rows are written with
// level.hip's slots: a 16-byte word wholly inside the tile's part of the row is one store, the ends go element by element.
#include <math.h>

#include "fh_common.h"
#include "truepeak_common.h"

namespace {

using namespace tp;                             // (truepeak_common.h: what stream_delivery.hip shares, the tile's constants too)
constexpr int MAX_LEN = 1 << 30;

struct tp_row {                                 // one row as the true-peak body sees it
  const float* x;
  int len;
};
struct BatchedRows {
  const float* x;
  int len;
  __device__ tp_row operator()(int r) const { return {x + (size_t)r * len, len}; }
};
struct ClipRows {                               // row r is channel (r - first row of its clip) of clip group[r] of the table
  const fh_pcm_clip* clips;
  const int32_t* group;
  int n_clips, max_len;
  __device__ tp_row operator()(int r) const {
    const int g = group[r];
    if (g < 0 || g >= n_clips) return {nullptr, 0};                 // (the tables live on the device: checked)
    int ch = 0;
    while (ch < r && group[r - ch - 1] == g) ++ch;
    const fh_pcm_clip c = clips[g];
    if (ch >= c.channels || c.len < 1 || c.len > max_len || !c.src) return {nullptr, 0};
    return {c.src + (long long)ch * c.pitch, c.len};
  }
};

struct tp_view {                                // one clip as the envelope and limiter bodies see it
  const float* src;                             // row c at src + c * pitch
  float* dst;                                   // row c at dst + c * dst_pitch (the limiter; may be the source rows themselves)
  long long pitch, dst_pitch;
  int channels, len;
};
struct BatchedClips {                           // equal clips back to back
  const float* x;
  float* y;
  int channels, len;
  __device__ tp_view operator()(int b) const {
    const size_t per = (size_t)channels * len;
    return {x + b * per, y ? y + b * per : nullptr, (long long)len, (long long)len, channels, len};
  }
};
struct ClipTable {                              // one fh_pcm_clip per clip on the device; dst NULL: in place
  const fh_pcm_clip* clips;
  int max_len;
  __device__ tp_view operator()(int b) const {
    const fh_pcm_clip c = clips[b];
    if (!c.src || c.len > max_len) return {nullptr, nullptr, 0, 0, 0, 0};
    float* d = reinterpret_cast<float*>(c.dst);
    return {c.src, d ? d : const_cast<float*>(c.src), (long long)c.pitch, d ? (long long)c.len : (long long)c.pitch, c.channels,
            c.len};
  }
};

// v[k] = max(|x[n]|, |x4[4 n + p]|, p = 0 .. 3) of frame n = tile0 + threadIdx.x + k * THREADS of the row x[0 .. len), 0 past its end.
// Ends with a barrier: xs may be staged again at once.  (hs is ready: the barrier behind the staging comes before its first read.)
__device__ __forceinline__ void tp_tile(const float* __restrict__ x, int len, int tile0, float* __restrict__ xs,
                                        const float (*hs)[PHASE_TAPS], float (&v)[PER]) {
  for (int j = threadIdx.x; j < TILE + 2 * HALO; j += THREADS) {
    const long long n = (long long)tile0 - HALO + j;
    xs[j] = (n >= 0 && n < len) ? x[n] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = threadIdx.x + k * THREADS;
    const float best = peak_at(xs, hs, i);
    v[k] = (tile0 + i < len) ? best : 0.f;
  }
  __syncthreads();
}

template <class Loc>
__global__ __launch_bounds__(THREADS) void true_peak_kernel(Loc loc, const float* __restrict__ taps, uint32_t* __restrict__ peak_bits) {
  __shared__ float xs[TILE + 2 * HALO];
  __shared__ float hs[4][PHASE_TAPS];
  __shared__ float wmax[THREADS / 64];
  const tp_row row = loc(blockIdx.y);
  const long long tile0 = (long long)blockIdx.x * TILE;
  if (row.len < 1 || tile0 >= row.len) return;
  load_taps(taps, hs);
  float v[PER];
  tp_tile(row.x, row.len, (int)tile0, xs, hs, v);
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) m = fmaxf(m, v[k]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) m = fmaxf(m, wmax[w]);
    atomicMax(&peak_bits[blockIdx.y], __float_as_uint(m));          // (non-negative float bits order as integers)
  }
}

template <class Loc>
__global__ __launch_bounds__(THREADS) void tp_envelope_kernel(Loc loc, const float* __restrict__ taps, float* __restrict__ m,
                                                              int m_pitch) {
  __shared__ float xs[TILE + 2 * HALO];
  __shared__ float hs[4][PHASE_TAPS];
  const tp_view c = loc(blockIdx.y);
  const long long tile0 = (long long)blockIdx.x * TILE;
  if (c.channels < 1 || c.channels > 8 || c.len < 1 || c.len > m_pitch || tile0 >= c.len) return;
  load_taps(taps, hs);
  float best[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) best[k] = 0.f;
  for (int ch = 0; ch < c.channels; ++ch) {
    float v[PER];
    tp_tile(c.src + (long long)ch * c.pitch, c.len, (int)tile0, xs, hs, v);
#pragma unroll
    for (int k = 0; k < PER; ++k) best[k] = fmaxf(best[k], v[k]);
  }
  float* __restrict__ out = m + (size_t)blockIdx.y * m_pitch + tile0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = threadIdx.x + k * THREADS;
    if (tile0 + i < c.len) out[i] = best[k];
  }
}

template <class Loc>
__global__ __launch_bounds__(THREADS) void limit_kernel(Loc loc, const float* __restrict__ m, int m_pitch,
                                                        const double* __restrict__ w, float* __restrict__ gain, int H, float c32) {
  __shared__ float a[2][LIM_N];
  __shared__ double ws[2 * MAX_H + 1];
  __shared__ float gs[TILE];
  const tp_view c = loc(blockIdx.y);
  const long long tile0 = (long long)blockIdx.x * TILE;
  if (c.channels < 1 || c.channels > 8 || c.len < 1 || c.len > m_pitch || tile0 >= c.len) return;
  const int t = threadIdx.x, N = TILE + 4 * H;
  const float* __restrict__ mc = m + (size_t)blockIdx.y * m_pitch;
  for (int j = t; j < N; j += THREADS) {                            // a[0][j] = r[tile0 - 2 H + j]
    const long long n = tile0 - 2 * H + j;
    float r = 1.f;
    if (n >= 0 && n < c.len) {
      const float mv = mc[n];
      if (mv > c32) r = __fdiv_rn(c32, mv);
    }
    a[0][j] = r;
  }
  for (int j = t; j < 2 * H + 1; j += THREADS) ws[j] = w[j];
  __syncthreads();
  double acc[PER];
  gain_tile(a, ws, H, acc);
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = t + k * THREADS;
    const float g = (float)acc[k];
    gs[i] = g;
    if (gain && tile0 + i < c.len) gain[(size_t)blockIdx.y * m_pitch + tile0 + i] = g;
  }
  __syncthreads();
  const int n_tile = (int)min((long long)TILE, c.len - tile0);
  for (int ch = 0; ch < c.channels; ++ch) {
    const float* src = c.src + (long long)ch * c.pitch + tile0;     // (in place: src and dst are the same elements, each read and
    float* dst = c.dst + (long long)ch * c.dst_pitch + tile0;       //  written by one thread)
    const int lead = (int)(((size_t)dst >> 2) & 3);                 // elements between the aligned address and the tile's part
    for (int s = t; s < TILE / 4 + 1; s += THREADS) {
      const int first = 4 * s - lead;
      if (first >= n_tile) break;
      if (first >= 0 && first + 4 <= n_tile) {
        f32x4 x;
        if ((((size_t)(src + first)) & 15) == 0) {
          x = *reinterpret_cast<const f32x4*>(src + first);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) x[k] = src[first + k];
        }
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = limit_sample(x[k], gs[first + k], c32);
        *reinterpret_cast<f32x4*>(dst + first) = y;
        continue;
      }
      for (int k = 0; k < 4; ++k) {
        const int j = first + k;
        if (j >= 0 && j < n_tile) dst[j] = limit_sample(src[j], gs[j], c32);
      }
    }
  }
}

// One thread per clip: the thread of a clip's first row reads the clip's loudness and the peaks of its rows (a clip's channels: a
// handful) and writes the gain into each of its rows.
__global__ __launch_bounds__(256) void delivery_gain_kernel(const float* __restrict__ lufs, double target,
                                                            const uint32_t* __restrict__ peak_bits,
                                                            const uint32_t* __restrict__ tp_bits, const int32_t* __restrict__ group,
                                                            int rows, int n_clips, double ceiling, int uncapped,
                                                            float* __restrict__ gains, float* __restrict__ dbtp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const int32_t g = group[i];
  if (g < 0 || g >= n_clips || (i > 0 && group[i - 1] == g)) return;
  uint32_t pk = 0, tp = 0;
  int end = i;
  for (; end < rows && group[end] == g; ++end) {                    // (non-negative float bits order as integers)
    if (peak_bits) pk = max(pk, peak_bits[end]);
    if (tp_bits) tp = max(tp, tp_bits[end]);
  }
  float gl = 1.f;
  if (target == target && lufs) {
    const float L = lufs[g];                                        // (the float32 that measure_loudness reports)
    if (isfinite(L)) {
      const double want = pow(10.0, (target - (double)L) / 20.0);
      if (uncapped) {
        gl = (float)want;
      } else {
        const double peak = (double)__uint_as_float(pk);
        if (isfinite(peak) && peak > 0.0) gl = (float)fmin(want, 0.99 / peak);
      }
    }
  }
  const double TP = (double)__uint_as_float(tp);
  float out = gl;
  if (!uncapped && tp_bits && TP > 0.0) out = (float)fmin((double)gl, ceiling / TP);
  if (gains)
    for (int r = i; r < end; ++r) gains[r] = out;
  if (dbtp) dbtp[g] = TP > 0.0 ? (float)(20.0 * log10(TP)) : -INFINITY;
}

int tiles(int len) { return fh_cdiv(len, TILE); }

bool aligned4(const void* p) { return (((size_t)p) & 3) == 0; }

}  // namespace

extern "C" int fh_tp_tile_len(void) { return TILE; }

extern "C" int fh_true_peak_f32(const float* x, const float* taps, uint32_t* peak_bits, int rows, int len, void* stream) {
  FH_CHECK_ARG(x && taps && peak_bits, "fh_true_peak_f32: null pointer (x %p, taps %p, peak_bits %p)", (const void*)x,
               (const void*)taps, (void*)peak_bits);
  FH_CHECK_ARG(rows > 0 && rows < 65536, "fh_true_peak_f32: %d rows (1 .. 65535)", rows);
  FH_CHECK_ARG(len > 0 && len <= MAX_LEN, "fh_true_peak_f32: len %d (1 .. 2^30)", len);
  FH_CHECK_ARG(aligned4(x) && aligned4(taps) && aligned4(peak_bits), "fh_true_peak_f32: x, taps and peak_bits must be 4-byte aligned");
  hipLaunchKernelGGL(true_peak_kernel<BatchedRows>, dim3(tiles(len), rows), dim3(THREADS), 0, (hipStream_t)stream,
                     BatchedRows{x, len}, taps, peak_bits);
  FH_CHECK_LAUNCH("fh_true_peak_f32");
  return FH_OK;
}

extern "C" int fh_true_peak_seg_f32(const fh_pcm_clip* clips, const int32_t* group, int n_clips, int rows, int max_len,
                                    const float* taps, uint32_t* peak_bits, void* stream) {
  FH_CHECK_ARG(clips && group && taps && peak_bits, "fh_true_peak_seg_f32: null pointer (clips %p, group %p, taps %p, peak_bits %p)",
               (const void*)clips, (const void*)group, (const void*)taps, (void*)peak_bits);
  FH_CHECK_ARG(n_clips > 0 && n_clips <= rows && rows < 65536, "fh_true_peak_seg_f32: %d clips of %d rows (1 <= clips <= rows "
               "<= 65535)", n_clips, rows);
  FH_CHECK_ARG(max_len > 0 && max_len <= MAX_LEN, "fh_true_peak_seg_f32: max_len %d (1 .. 2^30)", max_len);
  FH_CHECK_ARG(aligned4(taps) && aligned4(peak_bits), "fh_true_peak_seg_f32: taps and peak_bits must be 4-byte aligned");
  hipLaunchKernelGGL(true_peak_kernel<ClipRows>, dim3(tiles(max_len), rows), dim3(THREADS), 0, (hipStream_t)stream,
                     ClipRows{clips, group, n_clips, max_len}, taps, peak_bits);
  FH_CHECK_LAUNCH("fh_true_peak_seg_f32");
  return FH_OK;
}

extern "C" int fh_tp_envelope_f32(const float* x, const float* taps, float* m, int n_clips, int channels, int len, void* stream) {
  FH_CHECK_ARG(x && taps && m, "fh_tp_envelope_f32: null pointer (x %p, taps %p, m %p)", (const void*)x, (const void*)taps, (void*)m);
  FH_CHECK_ARG(n_clips > 0 && n_clips < 65536, "fh_tp_envelope_f32: %d clips (1 .. 65535)", n_clips);
  FH_CHECK_ARG(channels >= 1 && channels <= 8, "fh_tp_envelope_f32: %d channels (1 .. 8)", channels);
  FH_CHECK_ARG(len > 0 && len <= MAX_LEN, "fh_tp_envelope_f32: len %d (1 .. 2^30)", len);
  FH_CHECK_ARG(aligned4(x) && aligned4(taps) && aligned4(m), "fh_tp_envelope_f32: x, taps and m must be 4-byte aligned");
  hipLaunchKernelGGL(tp_envelope_kernel<BatchedClips>, dim3(tiles(len), n_clips), dim3(THREADS), 0, (hipStream_t)stream,
                     BatchedClips{x, nullptr, channels, len}, taps, m, len);
  FH_CHECK_LAUNCH("fh_tp_envelope_f32");
  return FH_OK;
}

extern "C" int fh_tp_envelope_seg_f32(const fh_pcm_clip* clips, int n_clips, int max_len, const float* taps, float* m,
                                      void* stream) {
  FH_CHECK_ARG(clips && taps && m, "fh_tp_envelope_seg_f32: null pointer (clips %p, taps %p, m %p)", (const void*)clips,
               (const void*)taps, (void*)m);
  FH_CHECK_ARG(n_clips > 0 && n_clips < 65536, "fh_tp_envelope_seg_f32: %d clips (1 .. 65535)", n_clips);
  FH_CHECK_ARG(max_len > 0 && max_len <= MAX_LEN, "fh_tp_envelope_seg_f32: max_len %d (1 .. 2^30)", max_len);
  FH_CHECK_ARG(aligned4(taps) && aligned4(m), "fh_tp_envelope_seg_f32: taps and m must be 4-byte aligned");
  hipLaunchKernelGGL(tp_envelope_kernel<ClipTable>, dim3(tiles(max_len), n_clips), dim3(THREADS), 0, (hipStream_t)stream,
                     ClipTable{clips, max_len}, taps, m, max_len);
  FH_CHECK_LAUNCH("fh_tp_envelope_seg_f32");
  return FH_OK;
}

#define FH_CHECK_LIMIT(name)                                                                                              \
  FH_CHECK_ARG(H >= 1 && H <= MAX_H, name ": H %d (1 .. %d)", H, MAX_H);                                                   \
  FH_CHECK_ARG(ceiling > 0.f && ceiling <= 1.f, name ": ceiling %g (0 < c <= 1)", (double)ceiling);                       \
  FH_CHECK_ARG(aligned4(m) && (((size_t)w) & 7) == 0 && aligned4(gain), name ": m and gain must be 4-byte, w 8-byte aligned")

extern "C" int fh_limit_f32(const float* x, float* y, const float* m, const double* w, float* gain, int n_clips, int channels,
                            int len, int H, float ceiling, void* stream) {
  FH_CHECK_ARG(x && y && m && w, "fh_limit_f32: null pointer (x %p, y %p, m %p, w %p)", (const void*)x, (void*)y, (const void*)m,
               (const void*)w);
  FH_CHECK_ARG(n_clips > 0 && n_clips < 65536, "fh_limit_f32: %d clips (1 .. 65535)", n_clips);
  FH_CHECK_ARG(channels >= 1 && channels <= 8, "fh_limit_f32: %d channels (1 .. 8)", channels);
  FH_CHECK_ARG(len > 0 && len <= MAX_LEN, "fh_limit_f32: len %d (1 .. 2^30)", len);
  FH_CHECK_ARG(aligned4(x) && aligned4(y), "fh_limit_f32: x and y must be 4-byte aligned");
  FH_CHECK_LIMIT("fh_limit_f32");
  hipLaunchKernelGGL(limit_kernel<BatchedClips>, dim3(tiles(len), n_clips), dim3(THREADS), 0, (hipStream_t)stream,
                     BatchedClips{x, y, channels, len}, m, len, w, gain, H, ceiling);
  FH_CHECK_LAUNCH("fh_limit_f32");
  return FH_OK;
}

extern "C" int fh_limit_seg_f32(const fh_pcm_clip* clips, int n_clips, int max_len, const float* m, const double* w, float* gain,
                                int H, float ceiling, void* stream) {
  FH_CHECK_ARG(clips && m && w, "fh_limit_seg_f32: null pointer (clips %p, m %p, w %p)", (const void*)clips, (const void*)m,
               (const void*)w);
  FH_CHECK_ARG(n_clips > 0 && n_clips < 65536, "fh_limit_seg_f32: %d clips (1 .. 65535)", n_clips);
  FH_CHECK_ARG(max_len > 0 && max_len <= MAX_LEN, "fh_limit_seg_f32: max_len %d (1 .. 2^30)", max_len);
  FH_CHECK_LIMIT("fh_limit_seg_f32");
  hipLaunchKernelGGL(limit_kernel<ClipTable>, dim3(tiles(max_len), n_clips), dim3(THREADS), 0, (hipStream_t)stream,
                     ClipTable{clips, max_len}, m, max_len, w, gain, H, ceiling);
  FH_CHECK_LAUNCH("fh_limit_seg_f32");
  return FH_OK;
}

extern "C" int fh_delivery_gain_f32(const float* lufs, double target, const uint32_t* peak_bits, const uint32_t* tp_bits,
                                    const int32_t* group, int rows, int n_clips, double ceiling, int uncapped, float* gains,
                                    float* dbtp, void* stream) {
  FH_CHECK_ARG(group && (gains || dbtp), "fh_delivery_gain_f32: null pointer (group %p, gains %p, dbtp %p)", (const void*)group,
               (void*)gains, (void*)dbtp);
  FH_CHECK_ARG(n_clips > 0 && n_clips <= rows && rows < 65536, "fh_delivery_gain_f32: %d clips of %d rows (1 <= clips <= rows "
               "<= 65535)", n_clips, rows);
  FH_CHECK_ARG(target != target || (target >= -70.0 && target <= 0.0 && lufs && (uncapped || peak_bits)),
               "fh_delivery_gain_f32: target %g LUFS (-70 .. 0 with lufs and, capped, peak_bits; or NaN: no loudness term)", target);
  FH_CHECK_ARG(uncapped || !tp_bits || (ceiling > 0.0 && ceiling <= 1.0), "fh_delivery_gain_f32: ceiling %g (0 < c <= 1)", ceiling);
  FH_CHECK_ARG(!uncapped || !tp_bits || dbtp, "fh_delivery_gain_f32: the uncapped rule does not read tp_bits");
  hipLaunchKernelGGL(delivery_gain_kernel, dim3(fh_cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, lufs, target, peak_bits,
                     tp_bits, group, rows, n_clips, ceiling, uncapped ? 1 : 0, gains, dbtp);
  FH_CHECK_LAUNCH("fh_delivery_gain_f32");
  return FH_OK;
}
