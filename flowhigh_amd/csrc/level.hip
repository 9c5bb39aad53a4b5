// Level-true output and multichannel clips (FlowHighSR.generate*(channels=, level=)): the per-row gains around the mono path.
//   fh_channel_peaks_f32   the resampler's peak slots -> the rows' gains p_c; a silent row's slot becomes 1.0 (its condition is
//                          then exact zeros instead of 0 / 0)
//   fh_row_gain_*          u_c = w_c * p_c on the iSTFT output: the signal at the input's own level
//   fh_group_peak_f32      G = max over a clip's channels of fl(q_c * p_c) into every row's peak slot, for fh_peak_scale_*_f32
// Peaks are non-negative float bits in uint32 slots, as fh_peak_abs_f32 / fh_istft_ola_f32 leave them.  Nothing here syncs.
#include "fh_common.h"

namespace {

constexpr uint32_t ONE_BITS = 0x3f800000u;        // 1.0f
constexpr uint32_t ABS_MASK = 0x7fffffffu;

// (the zero tests are on the bits: a denormal peak is a peak, whatever the denormal mode of the compare)
__global__ __launch_bounds__(256) void channel_peaks_kernel(uint32_t* __restrict__ peak_bits, float* __restrict__ gains, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = peak_bits[i];
  gains[i] = __uint_as_float(p);
  if ((p & ABS_MASK) == 0) peak_bits[i] = ONE_BITS;
}

// One thread per GROUP: the thread of a group's first row reads the q's and gains of its rows and writes their slots; no
// other thread touches them, so the update in place needs no second buffer (a group is a clip's channels: a handful of rows).
__global__ __launch_bounds__(256) void group_peak_kernel(uint32_t* __restrict__ q_bits, const float* __restrict__ gains,
                                                         const int32_t* __restrict__ group, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t g = group[i];
  if (i > 0 && group[i - 1] == g) return;
  float m = 0.f;
  int end = i;
  for (; end < n && group[end] == g; ++end) {
    const float gain = gains[end];
    if ((__float_as_uint(gain) & ABS_MASK) == 0) continue;          // a silent row: its q (anything, a NaN too) does not count
    m = fmaxf(m, __fmul_rn(__uint_as_float(q_bits[end]), gain));
  }
  const uint32_t out = m > 0.f ? __float_as_uint(m) : ONE_BITS;
  for (int r = i; r < end; ++r) q_bits[r] = out;
}

// row[0 .. len) *= g.  Slot s is the 16-byte word s of the row's memory counted from the aligned address at or below `row`:
// a slot wholly inside the row is one 16-byte access, the (at most two) slots that overlap an end go element by element.
__device__ __forceinline__ void row_gain_body(float* __restrict__ row, int len, float g) {
  const int lead = (int)(((size_t)row >> 2) & 3);                    // elements between the aligned address and the row
  const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * 4 - lead;      // the slot's first element in the row
  if (first >= len) return;
  if (first >= 0 && first + 4 <= len) {
    f32x4* p = reinterpret_cast<f32x4*>(row + first);
    *p = *p * g;
    return;
  }
  for (int k = 0; k < 4; ++k) {
    const long long j = first + k;
    if (j >= 0 && j < len) row[j] = row[j] * g;
  }
}

__global__ __launch_bounds__(256) void row_gain_kernel(float* __restrict__ y, const float* __restrict__ gains, int len) {
  row_gain_body(y + (size_t)blockIdx.y * len, len, gains[blockIdx.y]);
}

__global__ __launch_bounds__(256) void row_gain_seg_kernel(const fh_clip* __restrict__ clips, const float* __restrict__ gains) {
  const fh_clip c = clips[blockIdx.y];
  row_gain_body(c.dst, c.len_out, gains[blockIdx.y]);
}

int row_gain_blocks(int len) { return fh_cdiv(((long long)len + 3) / 4 + 1, 256); }      // slots of a row at any alignment

}  // namespace

extern "C" int fh_channel_peaks_f32(uint32_t* peak_bits, float* gains, int n, void* stream) {
  FH_CHECK_ARG(peak_bits && gains && n > 0, "fh_channel_peaks_f32: bad args");
  hipLaunchKernelGGL(channel_peaks_kernel, dim3(fh_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, peak_bits, gains, n);
  FH_CHECK_LAUNCH("fh_channel_peaks_f32");
  return FH_OK;
}

extern "C" int fh_group_peak_f32(uint32_t* q_bits, const float* gains, const int32_t* group, int n, void* stream) {
  FH_CHECK_ARG(q_bits && gains && group && n > 0, "fh_group_peak_f32: bad args");
  hipLaunchKernelGGL(group_peak_kernel, dim3(fh_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, q_bits, gains, group, n);
  FH_CHECK_LAUNCH("fh_group_peak_f32");
  return FH_OK;
}

extern "C" int fh_row_gain_f32(float* y, const float* gains, int batch, int len, void* stream) {
  FH_CHECK_ARG(y && gains && batch > 0 && batch < 65536 && len > 0, "fh_row_gain_f32: bad args (1 .. 65535 rows)");
  FH_CHECK_ARG((((size_t)y) & 3) == 0, "fh_row_gain_f32: y must be 4-byte aligned");
  hipLaunchKernelGGL(row_gain_kernel, dim3(row_gain_blocks(len), batch), dim3(256), 0, (hipStream_t)stream, y, gains, len);
  FH_CHECK_LAUNCH("fh_row_gain_f32");
  return FH_OK;
}

extern "C" int fh_row_gain_seg_f32(const fh_clip* clips, int n_clips, int max_len, const float* gains, void* stream) {
  FH_CHECK_ARG(clips && n_clips > 0 && n_clips < 65536, "fh_row_gain_seg_f32: bad clip table (1 .. 65535 clips)");
  FH_CHECK_ARG(gains && max_len > 0, "fh_row_gain_seg_f32: bad args");
  hipLaunchKernelGGL(row_gain_seg_kernel, dim3(row_gain_blocks(max_len), n_clips), dim3(256), 0, (hipStream_t)stream, clips,
                     gains);
  FH_CHECK_LAUNCH("fh_row_gain_seg_f32");
  return FH_OK;
}
