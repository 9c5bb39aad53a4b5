// Segment forms of the front / back end kernels of frontend.hip: clips of DIFFERENT lengths in one launch (the ragged
// serving path, FlowHighSR.generate_many(ends='ragged')).  Every clip gets the bits of the batched entry called on that clip
// alone: the per-element arithmetic is the one copy in frontend_elem.h, only the way a block finds its clip differs.
//
// fh_resample_poly_rates_seg_f32 also lets every clip have an INPUT RATE of its own: a row of filter constants per clip.
//
// Clips are described by the device int32 [n][2] table of (first row, rows) where rows are packed back to back (as
// fh_mel_energy_seg_f32 takes it), or by an fh_clip array where a clip has a pointer or a sample range of its own.
// Grid: clip on blockIdx.y (n_clips <= 65535), gridDim.x sized for the longest clip; blocks past a clip's end return at once.
#include "frontend_elem.h"

namespace {

__global__ __launch_bounds__(256) void resample_poly_seg_kernel(const fh_clip* __restrict__ clips,
                                                                const float* __restrict__ h, int up, int down,
                                                                int n_taps, int pre) {
  const fh_clip c = clips[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c.len_out) return;
  // h == nullptr: equal rates, a plain copy (the host gives len_in == len_out)
  c.dst[i] = h ? fe_resample_value(c.src, h, i, c.len_in, up, down, n_taps, pre) : (i < c.len_in ? c.src[i] : 0.f);
}

// resample_poly_seg_kernel where every clip has a rate of its own: clip c reads row rate_of[c] of `rates` and that row's taps
// in the bank.  The tables live on the device, so a block checks its row before it touches anything else and leaves its
// clip unwritten on a bad one (an index past the table, non-positive up / down, taps outside the bank).
__global__ __launch_bounds__(256) void resample_poly_rates_seg_kernel(const fh_clip* __restrict__ clips,
                                                                      const int32_t* __restrict__ rate_of,
                                                                      const fh_rate* __restrict__ rates, int n_rates,
                                                                      const float* __restrict__ tap_bank, int bank_len) {
  const int r = rate_of[blockIdx.y];
  if ((unsigned)r >= (unsigned)n_rates) return;
  const fh_rate q = rates[r];
  if (q.up <= 0 || q.down <= 0 || q.n_taps < 0 || q.taps_off < 0 || (long long)q.taps_off + q.n_taps > bank_len) return;
  const fh_clip c = clips[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c.len_out) return;
  // n_taps == 0: equal rates, a plain copy (the host gives len_in == len_out)
  c.dst[i] = q.n_taps ? fe_resample_value(c.src, tap_bank + q.taps_off, i, c.len_in, q.up, q.down, q.n_taps, q.n_pre_remove)
                      : (i < c.len_in ? c.src[i] : 0.f);
}

__global__ __launch_bounds__(256) void peak_abs_seg_kernel(const fh_clip* __restrict__ clips,
                                                           uint32_t* __restrict__ peak_bits) {
  const fh_clip c = clips[blockIdx.y];
  if ((int)blockIdx.x * 256 >= c.len_out) return;
  const float* xb = c.dst;
  float m = 0.f;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < c.len_out; j += gridDim.x * 256) m = fmaxf(m, fabsf(xb[j]));
  fe_block_peak(m, peak_bits + blockIdx.y);
}

__global__ __launch_bounds__(256) void peak_scale_seg_kernel(const fh_clip* __restrict__ clips,
                                                             const uint32_t* __restrict__ peak_bits, float target) {
  const fh_clip c = clips[blockIdx.y];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= c.len_out) return;
  const float peak = __uint_as_float(peak_bits[blockIdx.y]);
  c.dst[j] = fe_peak_scale_value(c.dst[j], peak, target);
}

__global__ __launch_bounds__(256) void frame_seg_kernel(const fh_clip* __restrict__ clips,
                                                        const float* __restrict__ window, float* __restrict__ frames,
                                                        int nfft, int hop, int pad, int pad_mode) {
  const fh_clip c = clips[blockIdx.y];
  const int t = blockIdx.x;
  if (t >= c.rows) return;
  float* f = frames + ((size_t)c.row0 + t) * nfft;
  for (int k = threadIdx.x; k < nfft; k += 256) f[k] = fe_frame_value(c.src, window, c.len_in, t, k, hop, pad, pad_mode);
}

__global__ __launch_bounds__(32 * FE_SE_LANES) void spec_energy_seg_kernel(const float* __restrict__ spec,
                                                                           float* __restrict__ energy,
                                                                           const int32_t* __restrict__ seg) {
  const int b = blockIdx.y;
  fe_spec_energy_block(spec + (size_t)seg[2 * b] * FE_P_WIDTH, energy + b * 1025, seg[2 * b + 1], blockIdx.x);
}

__global__ __launch_bounds__(256) void spec_splice_seg_kernel(const float* __restrict__ pred,
                                                              const float* __restrict__ src,
                                                              const int32_t* __restrict__ cr, float* __restrict__ out,
                                                              const int32_t* __restrict__ seg) {
  const int b = blockIdx.y;
  const size_t per_clip = (size_t)seg[2 * b + 1] * FE_P_WIDTH;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= per_clip) return;
  const int bin = fe_p_bin((int)(idx % FE_P_WIDTH));
  const size_t g = (size_t)seg[2 * b] * FE_P_WIDTH + idx;
  out[g] = bin < cr[b] ? src[g] : pred[g];
}

__global__ __launch_bounds__(256) void istft_ola_seg_kernel(const float* __restrict__ frames,
                                                            const float* __restrict__ window,
                                                            const fh_clip* __restrict__ clips,
                                                            uint32_t* __restrict__ peak_bits, int nfft, int hop) {
  const fh_clip c = clips[blockIdx.y];
  if ((int)blockIdx.x * 256 >= c.len_out) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  float v = 0.f;
  if (j < c.len_out) {
    v = fe_istft_ola_value(frames + (size_t)c.row0 * nfft, window, j, c.rows, nfft, hop);
    c.dst[j] = v;
  }
  fe_block_peak(fabsf(v), peak_bits + blockIdx.y);
}

// dst[ch * rows + n] = mel[(row0 + n) * d + ch]: 32 x 32 tiles through LDS, reads and writes both along the fast axis
__global__ __launch_bounds__(256) void rows_to_channels_seg_kernel(const float* __restrict__ mel,
                                                                   const fh_clip* __restrict__ clips, int d,
                                                                   int d_tiles) {
  __shared__ float tile[32][33];
  const fh_clip c = clips[blockIdx.y];
  const int n0 = ((int)blockIdx.x / d_tiles) * 32, c0 = ((int)blockIdx.x % d_tiles) * 32;
  if (n0 >= c.rows) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int n = n0 + r, ch = c0 + tx;
    tile[r][tx] = (n < c.rows && ch < d) ? mel[((size_t)c.row0 + n) * d + ch] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int ch = c0 + r, n = n0 + tx;
    if (ch < d && n < c.rows) c.dst[(size_t)ch * c.rows + n] = tile[tx][r];
  }
}

}  // namespace

extern "C" int fh_sizeof_clip(void) { return (int)sizeof(fh_clip); }

#define FH_CHECK_CLIPS(name) \
  FH_CHECK_ARG(clips && n_clips > 0 && n_clips < 65536, name ": bad clip table (1 .. 65535 clips)")

extern "C" int fh_resample_poly_seg_f32(const fh_clip* clips, int n_clips, int max_len_out, const float* taps, int up,
                                        int down, int n_taps, int n_pre_remove, void* stream) {
  FH_CHECK_CLIPS("fh_resample_poly_seg_f32");
  FH_CHECK_ARG(max_len_out > 0 && up > 0 && down > 0, "fh_resample_poly_seg_f32: bad args");
  FH_CHECK_ARG(taps ? n_taps > 0 : (up == 1 && down == 1), "fh_resample_poly_seg_f32: no taps for %d / %d", up, down);
  hipLaunchKernelGGL(resample_poly_seg_kernel, dim3(fh_cdiv(max_len_out, 256), n_clips), dim3(256), 0,
                     (hipStream_t)stream, clips, taps, up, down, n_taps, n_pre_remove);
  FH_CHECK_LAUNCH("fh_resample_poly_seg_f32");
  return FH_OK;
}

extern "C" int fh_sizeof_rate(void) { return (int)sizeof(fh_rate); }

extern "C" int fh_resample_poly_rates_seg_f32(const fh_clip* clips, const int32_t* rate_of, int n_clips, int max_len_out,
                                              const fh_rate* rates, int n_rates, const float* tap_bank, int bank_len,
                                              void* stream) {
  FH_CHECK_CLIPS("fh_resample_poly_rates_seg_f32");
  FH_CHECK_ARG(rate_of && rates && n_rates >= 1, "fh_resample_poly_rates_seg_f32: bad rate table (rate_of, rates, n_rates >= 1)");
  FH_CHECK_ARG(max_len_out > 0, "fh_resample_poly_rates_seg_f32: bad max_len_out %d", max_len_out);
  FH_CHECK_ARG(bank_len >= 0 && (tap_bank || bank_len == 0), "fh_resample_poly_rates_seg_f32: bad tap bank (%d floats)",
               bank_len);
  hipLaunchKernelGGL(resample_poly_rates_seg_kernel, dim3(fh_cdiv(max_len_out, 256), n_clips), dim3(256), 0,
                     (hipStream_t)stream, clips, rate_of, rates, n_rates, tap_bank, bank_len);
  FH_CHECK_LAUNCH("fh_resample_poly_rates_seg_f32");
  return FH_OK;
}

extern "C" int fh_peak_abs_seg_f32(const fh_clip* clips, int n_clips, int max_len, uint32_t* peak_bits, void* stream) {
  FH_CHECK_CLIPS("fh_peak_abs_seg_f32");
  FH_CHECK_ARG(peak_bits && max_len > 0, "fh_peak_abs_seg_f32: bad args");
  int bx = fh_cdiv(max_len, 256);
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(peak_abs_seg_kernel, dim3(bx, n_clips), dim3(256), 0, (hipStream_t)stream, clips, peak_bits);
  FH_CHECK_LAUNCH("fh_peak_abs_seg_f32");
  return FH_OK;
}

extern "C" int fh_peak_scale_seg_f32(const fh_clip* clips, int n_clips, int max_len, const uint32_t* peak_bits,
                                     float target, void* stream) {
  FH_CHECK_CLIPS("fh_peak_scale_seg_f32");
  FH_CHECK_ARG(peak_bits && max_len > 0, "fh_peak_scale_seg_f32: bad args");
  hipLaunchKernelGGL(peak_scale_seg_kernel, dim3(fh_cdiv(max_len, 256), n_clips), dim3(256), 0, (hipStream_t)stream,
                     clips, peak_bits, target);
  FH_CHECK_LAUNCH("fh_peak_scale_seg_f32");
  return FH_OK;
}

extern "C" int fh_frame_seg_f32(const fh_clip* clips, int n_clips, int max_rows, int min_len, const float* window,
                                float* frames, int nfft, int hop, int pad, int pad_mode, void* stream) {
  FH_CHECK_CLIPS("fh_frame_seg_f32");
  FH_CHECK_ARG(window && frames && max_rows > 0 && min_len > 0 && nfft > 0 && hop > 0 && pad >= 0 &&
               (pad_mode == 0 || pad_mode == 1), "fh_frame_seg_f32: bad args");
  FH_CHECK_ARG(pad_mode == 1 || pad < min_len, "fh_frame_seg_f32: reflect pad %d needs len > pad", pad);
  hipLaunchKernelGGL(frame_seg_kernel, dim3(max_rows, n_clips), dim3(256), 0, (hipStream_t)stream, clips, window,
                     frames, nfft, hop, pad, pad_mode);
  FH_CHECK_LAUNCH("fh_frame_seg_f32");
  return FH_OK;
}

extern "C" int fh_spec_energy_seg_f32(const float* spec, float* energy, const int32_t* seg, int n_seg, void* stream) {
  FH_CHECK_ARG(spec && energy && seg && n_seg > 0 && n_seg < 65536, "fh_spec_energy_seg_f32: bad args");
  hipLaunchKernelGGL(spec_energy_seg_kernel, dim3(FE_P_BLOCKS, n_seg), dim3(32 * FE_SE_LANES), 0, (hipStream_t)stream,
                     spec, energy, seg);
  FH_CHECK_LAUNCH("fh_spec_energy_seg_f32");
  return FH_OK;
}

extern "C" int fh_spec_splice_seg_f32(const float* pred, const float* src, const int32_t* cr, float* out,
                                      const int32_t* seg, int n_seg, int max_rows, void* stream) {
  FH_CHECK_ARG(pred && src && cr && out && seg && n_seg > 0 && n_seg < 65536 && max_rows > 0,
               "fh_spec_splice_seg_f32: bad args");
  dim3 grid(fh_cdiv((long long)max_rows * FE_P_WIDTH, 256), n_seg);
  hipLaunchKernelGGL(spec_splice_seg_kernel, grid, dim3(256), 0, (hipStream_t)stream, pred, src, cr, out, seg);
  FH_CHECK_LAUNCH("fh_spec_splice_seg_f32");
  return FH_OK;
}

extern "C" int fh_istft_ola_seg_f32(const float* frames, const float* window, const fh_clip* clips, int n_clips,
                                    int max_len, uint32_t* peak_bits, int nfft, int hop, void* stream) {
  FH_CHECK_CLIPS("fh_istft_ola_seg_f32");
  FH_CHECK_ARG(frames && window && peak_bits && max_len > 0 && nfft > 0 && hop > 0, "fh_istft_ola_seg_f32: bad args");
  hipLaunchKernelGGL(istft_ola_seg_kernel, dim3(fh_cdiv(max_len, 256), n_clips), dim3(256), 0, (hipStream_t)stream,
                     frames, window, clips, peak_bits, nfft, hop);
  FH_CHECK_LAUNCH("fh_istft_ola_seg_f32");
  return FH_OK;
}

extern "C" int fh_rows_to_channels_seg_f32(const float* mel, const fh_clip* clips, int n_clips, int max_rows, int d,
                                           void* stream) {
  FH_CHECK_CLIPS("fh_rows_to_channels_seg_f32");
  FH_CHECK_ARG(mel && max_rows > 0 && d > 0, "fh_rows_to_channels_seg_f32: bad args");
  const int d_tiles = fh_cdiv(d, 32);
  hipLaunchKernelGGL(rows_to_channels_seg_kernel, dim3(fh_cdiv(max_rows, 32) * d_tiles, n_clips), dim3(256), 0,
                     (hipStream_t)stream, mel, clips, d, d_tiles);
  FH_CHECK_LAUNCH("fh_rows_to_channels_seg_f32");
  return FH_OK;
}
