// Spectral quality report on the device (FlowHighSR.measure_quality): log-spectral distance of an estimate from a reference, over
// all bins and below / above a cutoff bin, and their SNR, as flowhigh_amd/quality.py defines them.
//   fh_quality_frames_f32       float32 row pairs [rows, len] -> double [rows, F, 5]: per frame of the post-processing STFT
//                               (n_fft 2048, hop 480, zero pad 1024) the three band distances and the two SNR sums of its hop
//   fh_quality_frames_seg_f32   the same over a device table of clips read where they are (two pointers + two row pitches)
//   fh_quality_report_f32       the frames of every clip's rows -> its four figures
// The two frame entries are instantiations of one kernel body that differ in the row locator, so a row pair gets the same bits
// from each.  Everything behind the float32 loads is float64.
//
// One workgroup owns one frame of one row pair.  Both signals are read where they lie, with the zero pad and the window applied
// on the way into LDS: no frame tensor and no spectrum is stored (two [rows, 2048] and two [rows, 2112] float tensors, 33 KB per
// frame, against the 40 bytes per frame written here).  The estimate goes into the real part and the reference into the
// imaginary part of ONE 2048-point complex transform (fft2048.h, the 32 KB of LDS of fh_rfft2048_f32); with Z = FFT(e + i r)
//   X_e[k] = (Z[k] + conj Z[N - k]) / 2,   X_r[k] = (Z[k] - conj Z[N - k]) / (2 i),
// so a bin's two powers are read off Z[k] and Z[N - k].  The separation costs about 11 * 2^-52 * sqrt(P_r / P_e) in a bin's
// log-power difference, 3e-8 at the worst where one side is at the floor ("Quality report").
// Sums: a thread adds its bins k = tid, tid + 256, ... in ascending order, the 256 lanes are added in a fixed tree (wave
// butterfly, then the 4 waves in order).  No floating-point atomics anywhere.
#include <math.h>

#include "fft2048.h"

namespace {

constexpr int THREADS = 256;
constexpr int HOP = 480;
constexpr int PAD = FFT_N / 2;
constexpr int VALUES = 5;                       // l_full, l_low, l_high, sum r^2, sum (r - e)^2
constexpr int MAX_LEN = 1 << 30;
constexpr double FLOOR = 1e-8;                  // quality.FLOOR

// One row pair as the kernel body sees it; len < 1: nothing to do.
struct q_row {
  const float* e;
  const float* r;
  int len, kc;
  double* out;                                  // the row's frames, VALUES doubles each
};

__host__ __device__ inline bool kc_ok(int kc) { return kc >= -1 && kc <= FFT_BINS; }
__host__ __device__ inline bool clip_ok(const fh_quality_clip& c, int max_len) {
  return c.est && c.ref && c.channels >= 1 && c.len >= 1 && c.len <= max_len && kc_ok(c.kc);
}

struct BatchedPairs {
  const float* est;
  const float* ref;
  int len, kc;
  double* out;
  int f_pitch;
  __device__ q_row operator()(int r) const {
    return {est + (size_t)r * len, ref + (size_t)r * len, len, kc, out + (size_t)r * f_pitch * VALUES};
  }
};
struct ClipPairs {                              // row r is channel (r - first row of its clip) of clip group[r] of the table
  const fh_quality_clip* clips;
  const int32_t* group;
  int n_clips, max_len;
  double* out;
  int f_pitch;
  __device__ q_row operator()(int r) const {
    const int g = group[r];
    if (g < 0 || g >= n_clips) return {nullptr, nullptr, 0, 0, nullptr};          // (the tables live on the device: checked)
    int ch = 0;
    while (ch < r && group[r - ch - 1] == g) ++ch;
    const fh_quality_clip c = clips[g];
    if (!clip_ok(c, max_len) || ch >= c.channels) return {nullptr, nullptr, 0, 0, nullptr};   // (its row of `out` has max_len's frames)
    return {c.est + (long long)ch * c.est_pitch, c.ref + (long long)ch * c.ref_pitch, c.len, c.kc,
            out + (size_t)r * f_pitch * VALUES};
  }
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// N fixed-tree sums over the workgroup at once, the results in tot[] of thread 0 only (red [N][THREADS / 64]: LDS; one barrier)
template <int N>
__device__ __forceinline__ void block_sums_f64(double (&v)[N], double (*red)[THREADS / 64]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double w = wave_sum_f64(v[i]);
    if ((threadIdx.x & 63) == 0) red[i][threadIdx.x >> 6] = w;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = ((red[i][0] + red[i][1]) + red[i][2]) + red[i][3];
}

template <class Loc>
__global__ __launch_bounds__(THREADS) void quality_frames_kernel(Loc loc, const float* __restrict__ window,
                                                                 const double2* __restrict__ tw) {
  __shared__ double re[FFT_N];
  __shared__ double im[FFT_N];
  __shared__ double red[VALUES][THREADS / 64];
  const q_row row = loc(blockIdx.y);
  const int t = blockIdx.x, tid = threadIdx.x;
  if (row.len < 1 || t > row.len / HOP) return;                     // (the segment form's grid is sized for the longest clip)
  const int base = HOP * t - PAD;                                   // the frame's sample 0

  // e -> Re, r -> Im, windowed, in bit-reversed order; the frame owns the samples [HOP t, min(HOP t + HOP, len)): j in [PAD, PAD + HOP)
  double v[VALUES] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < FFT_N / THREADS; ++q) {
    const int j = tid + THREADS * q, i = base + j;
    const bool in = i >= 0 && i < row.len;
    const double xe = in ? (double)row.e[i] : 0.0, xr = in ? (double)row.r[i] : 0.0;
    const double w = (double)window[j];
    const int b = bitrev11(j);
    re[b] = xe * w;                                                 // (exact: 24 x 24 bits)
    im[b] = xr * w;
    if (in && j >= PAD && j < PAD + HOP) {
      const double dn = xr - xe;
      v[3] = fma(xr, xr, v[3]);
      v[4] = fma(dn, dn, v[4]);
    }
  }
  fft2048_stages(re, im, tw, tid);

  const int kc = row.kc;
  for (int k = tid; k < FFT_BINS; k += THREADS) {                   // (thread 0 has bin 1024 as well)
    const int nk = (FFT_N - k) & (FFT_N - 1);
    const double zr = re[k], zi = im[k], yr = re[nk], yi = im[nk];
    const double ea = zr + yr, eb = zi - yi;                        // 2 X_e = Z[k] + conj Z[N - k]
    const double ra = zi + yi, rb = yr - zr;                        // 2 X_r = (Z[k] - conj Z[N - k]) / i
    const double pe = 0.25 * fma(ea, ea, eb * eb), pr = 0.25 * fma(ra, ra, rb * rb);
    const double d = log10(fmax(pr, FLOOR)) - log10(fmax(pe, FLOOR));
    const double d2 = d * d;
    v[0] += d2;
    v[1] += k < kc ? d2 : 0.0;
    v[2] += k < kc ? 0.0 : d2;
  }
  block_sums_f64(v, red);
  if (tid == 0) {
    double* __restrict__ o = row.out + (size_t)t * VALUES;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    o[0] = sqrt(v[0] / (double)FFT_BINS);
    o[1] = kc < 0 ? nan : sqrt(v[1] / (double)kc);                  // (an empty band: 0 / 0)
    o[2] = kc < 0 ? nan : sqrt(v[2] / (double)(FFT_BINS - kc));
    o[3] = v[3];
    o[4] = v[4];
  }
}

// One workgroup per clip, its rows those r with group[r] == clip.
__global__ __launch_bounds__(THREADS) void quality_report_kernel(const double* __restrict__ frames, int f_pitch,
                                                                 const int32_t* __restrict__ lens, const int32_t* __restrict__ group,
                                                                 int rows, float* __restrict__ report) {
  __shared__ int first_row, n_rows;
  __shared__ double red[VALUES][THREADS / 64];
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
  float* __restrict__ out = report + 4 * (size_t)clip;
  const int T = C > 0 ? lens[r0] : 0;
  const int F = T > 0 ? 1 + T / HOP : 0;
  if (F < 1 || F > f_pitch) {                                       // (lens lives on the device: frames its row does not hold are not read)
    if (t < 4) out[t] = __int_as_float(0x7fc00000);
    return;
  }
  const long long n = (long long)C * F;
  double v[VALUES] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long i = t; i < n; i += THREADS) {
    const int c = (int)(i / F), f = (int)(i - (long long)c * F);
    const double* __restrict__ p = frames + ((size_t)(r0 + c) * f_pitch + f) * VALUES;
#pragma unroll
    for (int k = 0; k < VALUES; ++k) v[k] += p[k];
  }
  block_sums_f64(v, red);
  if (t == 0) {
    out[0] = (float)(v[0] / (double)n);
    out[1] = (float)(v[1] / (double)n);
    out[2] = (float)(v[2] / (double)n);
    out[3] = (float)(10.0 * log10(v[3] / v[4]));                    // (x / 0: +inf, 0 / x: -inf, 0 / 0: NaN)
  }
}

}  // namespace

extern "C" int fh_sizeof_quality_clip(void) { return (int)sizeof(fh_quality_clip); }

#define FH_CHECK_QUALITY_TABLES(name)                                                                                              \
  FH_CHECK_ARG(window && twiddles && frames, name ": null pointer (window %p, twiddles %p, frames %p)", (const void*)window,       \
               (const void*)twiddles, (void*)frames);                                                                              \
  FH_CHECK_ARG((((size_t)window) & 3) == 0 && (((size_t)twiddles) & 15) == 0 && (((size_t)frames) & 7) == 0,                       \
               name ": window must be 4-byte, twiddles 16-byte, frames 8-byte aligned")

extern "C" int fh_quality_frames_f32(const float* est, const float* ref, const float* window, const double* twiddles, double* frames,
                                     int rows, int len, int kc, void* stream) {
  FH_CHECK_ARG(est && ref, "fh_quality_frames_f32: null pointer (est %p, ref %p)", (const void*)est, (const void*)ref);
  FH_CHECK_QUALITY_TABLES("fh_quality_frames_f32");
  FH_CHECK_ARG(rows > 0 && rows < 65536, "fh_quality_frames_f32: %d rows (1 .. 65535)", rows);
  FH_CHECK_ARG(len >= 1 && len <= MAX_LEN, "fh_quality_frames_f32: len %d (1 .. 2^30)", len);
  FH_CHECK_ARG(kc_ok(kc), "fh_quality_frames_f32: kc %d (-1: no cutoff, 0 .. 1025)", kc);
  FH_CHECK_ARG((((size_t)est | (size_t)ref) & 3) == 0, "fh_quality_frames_f32: est and ref must be 4-byte aligned");
  const int F = 1 + len / HOP;
  hipLaunchKernelGGL(quality_frames_kernel<BatchedPairs>, dim3(F, rows), dim3(THREADS), 0, (hipStream_t)stream,
                     BatchedPairs{est, ref, len, kc, frames, F}, window, (const double2*)twiddles);
  FH_CHECK_LAUNCH("fh_quality_frames_f32");
  return FH_OK;
}

extern "C" int fh_quality_frames_seg_f32(const fh_quality_clip* clips, const fh_quality_clip* check, const int32_t* group, int n_clips,
                                         int rows, int max_len, const float* window, const double* twiddles, double* frames,
                                         void* stream) {
  FH_CHECK_ARG(clips && check && group, "fh_quality_frames_seg_f32: null pointer (clips %p, check %p, group %p)", (const void*)clips,
               (const void*)check, (const void*)group);
  FH_CHECK_QUALITY_TABLES("fh_quality_frames_seg_f32");
  FH_CHECK_ARG(n_clips > 0 && n_clips <= rows && rows < 65536, "fh_quality_frames_seg_f32: %d clips of %d rows (1 <= clips <= rows "
               "<= 65535)", n_clips, rows);
  FH_CHECK_ARG(max_len >= 1 && max_len <= MAX_LEN, "fh_quality_frames_seg_f32: max_len %d (1 .. 2^30)", max_len);
  for (int i = 0; i < n_clips; ++i) {
    const fh_quality_clip& c = check[i];
    FH_CHECK_ARG(kc_ok(c.kc), "fh_quality_frames_seg_f32: clip %d: kc %d (-1: no cutoff, 0 .. 1025)", i, c.kc);
    FH_CHECK_ARG(clip_ok(c, max_len), "fh_quality_frames_seg_f32: clip %d: len %d (1 .. max_len %d), %d channels (1 or more), or a null "
                 "pointer (est %p, ref %p)", i, c.len, max_len, c.channels, (const void*)c.est, (const void*)c.ref);
    FH_CHECK_ARG((((size_t)c.est | (size_t)c.ref) & 3) == 0, "fh_quality_frames_seg_f32: clip %d: est and ref must be 4-byte aligned", i);
  }
  const int F = 1 + max_len / HOP;
  hipLaunchKernelGGL(quality_frames_kernel<ClipPairs>, dim3(F, rows), dim3(THREADS), 0, (hipStream_t)stream,
                     ClipPairs{clips, group, n_clips, max_len, frames, F}, window, (const double2*)twiddles);
  FH_CHECK_LAUNCH("fh_quality_frames_seg_f32");
  return FH_OK;
}

extern "C" int fh_quality_report_f32(const double* frames, int f_pitch, const int32_t* lens, const int32_t* group, int rows,
                                     int n_clips, float* report, void* stream) {
  FH_CHECK_ARG(frames && lens && group && report, "fh_quality_report_f32: null pointer (frames %p, lens %p, group %p, report %p)",
               (const void*)frames, (const void*)lens, (const void*)group, (void*)report);
  FH_CHECK_ARG(n_clips > 0 && n_clips <= rows && rows < 65536, "fh_quality_report_f32: %d clips of %d rows (1 <= clips <= rows "
               "<= 65535)", n_clips, rows);
  FH_CHECK_ARG(f_pitch >= 1 && f_pitch <= 1 + MAX_LEN / HOP, "fh_quality_report_f32: f_pitch %d (1 .. 1 + 2^30 / 480)", f_pitch);
  FH_CHECK_ARG((((size_t)frames) & 7) == 0 && (((size_t)report) & 3) == 0,
               "fh_quality_report_f32: frames must be 8-byte, report 4-byte aligned");
  hipLaunchKernelGGL(quality_report_kernel, dim3(n_clips), dim3(THREADS), 0, (hipStream_t)stream, frames, f_pitch, lens, group, rows,
                     report);
  FH_CHECK_LAUNCH("fh_quality_report_f32");
  return FH_OK;
}
