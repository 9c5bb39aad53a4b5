// HBM-bound kernels either side of the DFT GEMMs: STFT framing, spectral energy / cutoff search,
// band splice, inverse-STFT overlap-add, peak normalisation, polyphase resampling.
//
// Replaces, in the reference (paths under its src/flowhigh/):
//   fh_frame_f32          F.pad(reflect) + the framing half of torch.stft   models/melvoco.py:74-79
//                         and of torchaudio Spectrogram (zero pad)           postprocessing.py:7,22-23
//   fh_spec_energy_f32 /  get_cutoff_index (a <=1025-iteration python loop
//   fh_cutoff_index_f32   with a host sync per iteration on GPU)             postprocessing.py:10-16
//   fh_spec_splice_f32    result[:cr] = src ; result[cr:] = pred            postprocessing.py:36-37
//   fh_istft_ola_f32      the overlap-add half of torch.istft               postprocessing.py:8,39
//   fh_peak_*             audio / max|audio| * 0.99 ; cond /= max|cond|      postprocessing.py:40, flowhighsr.py:69
//   fh_resample_poly_f32  scipy.signal.resample_poly (host numpy in the ref) flowhighsr.py:68
//
// Every step that works clip by clip is ONE kernel body with a clip locator as template parameter: the batched entries
// (equal-length clips, clip b at b * len) and their segment forms (fh_*_seg_f32: clips of DIFFERENT lengths in one launch, the
// ragged serving path, FlowHighSR.generate_many(ends='ragged')) are instantiations of it, so a clip gets the same bits
// whichever entry runs it.  Grid: clip on blockIdx.y (n_clips <= 65535); the segment forms size gridDim.x for the longest
// clip and blocks past a clip's end return at once.
#include "fh_common.h"

namespace {

constexpr int P_BLOCKS = 33;                // 33 * 32 = 1056 >= 1025 bins
constexpr int P_WIDTH = P_BLOCKS * 64;      // 2112 floats per frame (P-layout)

// ---- clip locators: passed to a kernel by value, loc(blockIdx.y) is the clip's view (a kernel reads only the fields its
// step needs).  kExact: gridDim.x is sized for this very clip, so no block lies wholly past its end.
struct BatchedClips {      // equal-length clips back to back: clip b is computed
  static constexpr bool kExact = true;
  const float* src;
  float* dst;
  int len_in, len_out, rows;
  __device__ fh_clip operator()(int b) const {
    return {src + (size_t)b * len_in, dst + (size_t)b * len_out, len_in, len_out, b * rows, rows};
  }
};
struct ClipTable {         // one fh_clip per clip on the device
  static constexpr bool kExact = false;
  const fh_clip* clips;
  __device__ fh_clip operator()(int b) const { return clips[b]; }
};
struct RowTable {          // device int32 [n][2] = (first row, rows): the steps that only touch packed rows
  static constexpr bool kExact = false;
  const int32_t* seg;
  __device__ fh_clip operator()(int b) const {
    unsigned long long r;      // (the pair as ONE 8-byte scalar load: two loads, of which the compiler sinks one, cost a second wait)
    __builtin_memcpy(&r, seg + 2 * b, 8);
    return {nullptr, nullptr, 0, 0, (int32_t)r, (int32_t)(r >> 32)};
  }
};
BatchedClips batched_rows(int rows) { return {nullptr, nullptr, 0, 0, rows}; }

// frames[row0 + t, k] = pad(src)[hop t + k] * window[k]; pad_mode 0: reflect (no edge repeat; pad < len), 1: zero
template <class Loc>
__global__ __launch_bounds__(256) void frame_kernel(Loc loc, const float* __restrict__ window, float* __restrict__ frames,
                                                    int nfft, int hop, int pad, int pad_mode) {
  const fh_clip c = loc(blockIdx.y);
  const int t = blockIdx.x;
  if (!Loc::kExact && t >= c.rows) return;
  float* f = frames + ((size_t)c.row0 + t) * nfft;
  for (int k = threadIdx.x; k < nfft; k += 256) {
    int i = hop * t + k - pad;
    float v;
    if (pad_mode == 0) {
      if (i < 0) i = -i;
      if (i >= c.len_in) i = 2 * (c.len_in - 1) - i;
      v = c.src[i];
    } else {
      v = (i >= 0 && i < c.len_in) ? c.src[i] : 0.f;
    }
    f[k] = v * window[k];
  }
}

// energy[b, bin] = sum_t |S[t, bin]| over the clip's rows.  grid (33, clips); thread -> (bin i = tid & 31, frame lane =
// tid >> 5); 32 frame lanes x 2 independent partial sums keep enough loads in flight (8 lanes with one dependent chain each
// took 46 us at B = 1): every lane sums its frames t = fl, fl + 64, ... and t = fl + 32, fl + 96, ... in double, lanes are
// added in lane order.
constexpr int SE_LANES = 32;
template <class Loc>
__global__ __launch_bounds__(32 * SE_LANES) void spec_energy_kernel(Loc loc, const float* __restrict__ spec,
                                                                    float* __restrict__ energy) {
  __shared__ double part[SE_LANES][32];
  const int b = blockIdx.y, blk = blockIdx.x;
  const fh_clip c = loc(b);
  const int i = threadIdx.x & 31, fl = threadIdx.x >> 5;
  const float* s = spec + (size_t)c.row0 * P_WIDTH + blk * 64;
  double acc = 0.0, acc2 = 0.0;
  for (int t = fl; t < c.rows; t += 2 * SE_LANES) {
    float re = s[(size_t)t * P_WIDTH + i], im = s[(size_t)t * P_WIDTH + 32 + i];
    acc += (double)sqrtf(re * re + im * im);
    const int t2 = t + SE_LANES;
    if (t2 < c.rows) {
      re = s[(size_t)t2 * P_WIDTH + i], im = s[(size_t)t2 * P_WIDTH + 32 + i];
      acc2 += (double)sqrtf(re * re + im * im);
    }
  }
  part[fl][i] = acc + acc2;
  __syncthreads();
  if (fl == 0) {
    double tot = 0.0;
#pragma unroll
    for (int q = 0; q < SE_LANES; ++q) tot += part[q][i];
    const int bin = blk * 32 + i;
    if (bin < 1025) energy[b * 1025 + bin] = (float)tot;
  }
}

// torch.cumsum on CPU accumulates float32 input in double and rounds every prefix to float;
// the threshold product is a float32 multiply (postprocessing.py:11-12).
__global__ __launch_bounds__(64) void cutoff_kernel(const float* __restrict__ energy, int32_t* __restrict__ cr,
                                                    int nbins, float thr) {
  // One wave per clip: lane l owns the contiguous chunk [l * per, (l + 1) * per) of the bins; chunk
  // sums are scanned across lanes in double, then every prefix is rounded to float exactly where the
  // sequential double accumulation of torch.cumsum would round it (same values up to 1e-16 relative).
  __shared__ float cum[1088];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int per = (nbins + 63) / 64;
  const int f0 = lane * per;
  double local = 0.0;
  for (int f = f0; f < f0 + per && f < nbins; ++f) local += (double)energy[b * nbins + f];
  double incl = local;                              // inclusive scan of the chunk sums
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  double c = incl - local;
  for (int f = f0; f < f0 + per && f < nbins; ++f) {
    c += (double)energy[b * nbins + f];
    cum[f] = (float)c;
  }
  __syncthreads();
  const float limit = cum[nbins - 1] * thr;
  // largest j in [1, nbins - 1] with cum[j] < limit, else 0
  int best = 0;
  for (int f = f0; f < f0 + per && f < nbins; ++f)
    if (f >= 1 && cum[f] < limit) best = f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if (lane == 0) cr[b] = best;
}

// energy[b, d] = sum_n exp(mel[b, n, d]) over the clip's own rows, in row order (locate_cutoff_freq on exp(mel),
// cfm_superresolution.py:134-159)
template <class Loc>
__global__ __launch_bounds__(256) void mel_energy_kernel(Loc loc, const float* __restrict__ mel,
                                                         float* __restrict__ energy, int d) {
  const int b = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= d) return;
  const fh_clip c = loc(b);
  const float* m = mel + (size_t)c.row0 * d + col;
  double acc = 0.0;
  for (int t = 0; t < c.rows; ++t) acc += (double)expf(m[(size_t)t * d]);
  energy[b * d + col] = (float)acc;
}

// out[b, n, d] = d < cut[b] ? low : high      (mel_replace_ops, cfm_superresolution.py:146-152)
template <class Loc>
__global__ __launch_bounds__(256) void mel_splice_kernel(Loc loc, const float* __restrict__ low,
                                                         const float* __restrict__ high,
                                                         const int32_t* __restrict__ cut, float* __restrict__ out, int d) {
  const int b = blockIdx.y;
  const fh_clip c = loc(b);
  const size_t per = (size_t)c.rows * d;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  const size_t g = (size_t)c.row0 * d + i;
  out[g] = (int)(i % d) < cut[b] ? low[g] : high[g];
}

__global__ __launch_bounds__(256) void axpby_kernel(const float* __restrict__ x, float a,
                                                    const float* __restrict__ y, float bcoef,
                                                    float* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = x[i] * a + y[i] * bcoef;      // cond * std_1 + epsilon * std_2 (cfm:226-236)
}

// out = bin < cr[b] ? src : pred on the clip's P-layout rows (re at 64 q + i, im at 64 q + 32 + i, bin = 32 q + i)
template <class Loc>
__global__ __launch_bounds__(256) void spec_splice_kernel(Loc loc, const float* __restrict__ pred,
                                                          const float* __restrict__ src,
                                                          const int32_t* __restrict__ cr, float* __restrict__ out) {
  const int b = blockIdx.y;
  const fh_clip c = loc(b);
  const size_t per_clip = (size_t)c.rows * P_WIDTH;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= per_clip) return;
  const int col = (int)(idx % P_WIDTH);
  const int bin = (col >> 6) * 32 + (col & 31);
  const size_t g = (size_t)c.row0 * P_WIDTH + idx;
  out[g] = bin < cr[b] ? src[g] : pred[g];
}

// max over a 256-thread block of m >= 0 into *peak_bits (non-negative float bits order as integers: order-independent)
__device__ __forceinline__ void block_peak(float m, uint32_t* __restrict__ peak_bits) {
  __shared__ float red[4];
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(peak_bits, __float_as_uint(m));
  }
}

// sample j of the inverse STFT's overlap-add over the clip's n_frames rows at `fb`: sum_t w f / sum_t w^2 over the frames
// that cover j, zero past the OLA signal's end (torch.istft zero-fills there)
__device__ __forceinline__ float istft_ola_value(const float* __restrict__ fb, const float* __restrict__ window, int j,
                                                 int n_frames, int nfft, int hop) {
  const int avail = hop * (n_frames - 1) + nfft / 2;
  if (j >= avail) return 0.f;
  const int p = j + nfft / 2;
  int t_hi = p / hop;
  if (t_hi > n_frames - 1) t_hi = n_frames - 1;
  int t_lo = (p - nfft + hop) / hop;          // ceil((p - nfft + 1) / hop) for p - nfft + 1 > 0
  if (p - nfft + 1 <= 0) t_lo = 0;
  float num = 0.f, den = 0.f;
  for (int t = t_lo; t <= t_hi; ++t) {
    const int k = p - hop * t;
    const float w = window[k];
    num = fmaf(w, fb[(size_t)t * nfft + k], num);
    den = fmaf(w, w, den);
  }
  return num / den;
}

template <class Loc>
__global__ __launch_bounds__(256) void istft_ola_kernel(Loc loc, const float* __restrict__ frames,
                                                        const float* __restrict__ window,
                                                        uint32_t* __restrict__ peak_bits, int nfft, int hop) {
  const fh_clip c = loc(blockIdx.y);
  if (!Loc::kExact && (int)blockIdx.x * 256 >= c.len_out) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  float v = 0.f;
  if (j < c.len_out) {
    v = istft_ola_value(frames + (size_t)c.row0 * nfft, window, j, c.rows, nfft, hop);
    c.dst[j] = v;
  }
  block_peak(fabsf(v), peak_bits + blockIdx.y);
}

// peak_bits[b] = bits(max |dst|); gridDim.x may be capped below the clip's blocks: a grid-stride loop
template <class Loc>
__global__ __launch_bounds__(256) void peak_abs_kernel(Loc loc, uint32_t* __restrict__ peak_bits) {
  const fh_clip c = loc(blockIdx.y);
  if (!Loc::kExact && (int)blockIdx.x * 256 >= c.len_out) return;
  const float* xb = c.dst;
  float m = 0.f;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < c.len_out; j += gridDim.x * 256) m = fmaxf(m, fabsf(xb[j]));
  block_peak(m, peak_bits + blockIdx.y);
}

// same order as the reference: (y / peak) * 0.99
template <class Loc>
__global__ __launch_bounds__(256) void peak_scale_kernel(Loc loc, const uint32_t* __restrict__ peak_bits, float target) {
  const fh_clip c = loc(blockIdx.y);
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= c.len_out) return;
  const float peak = __uint_as_float(peak_bits[blockIdx.y]);
  const float v = c.dst[j] / peak;
  c.dst[j] = v * target;
}

// ---- polyphase resampler.  A filter source is the kernel's second parameter: flt(b, f) gives clip b's filter constants,
// or false where the clip is to be left unwritten.  f.h == nullptr (kMayCopy sources only): equal rates, a plain copy (the
// host gives len_in == len_out).
struct fe_filter {
  const float* h;
  int up, down, n_taps, pre;
};
template <bool MAY_COPY>
struct LaunchFilter {      // one set of constants for the launch
  static constexpr bool kMayCopy = MAY_COPY;
  fe_filter f;
  __device__ bool operator()(int, fe_filter& out) const {
    out = f;
    return true;
  }
};
// Every clip a rate of its own: clip b reads row rate_of[b] of `rates` and that row's taps in the bank.  The tables live on
// the device, so a block checks its row before it touches anything else and leaves its clip unwritten on a bad one (an index
// past the table, non-positive up / down, taps outside the bank).  n_taps == 0: the copy.
struct RowFilter {
  static constexpr bool kMayCopy = true;
  const int32_t* rate_of;
  const fh_rate* rates;
  int n_rates;
  const float* tap_bank;
  int bank_len;
  __device__ bool operator()(int b, fe_filter& out) const {
    const int r = rate_of[b];
    if ((unsigned)r >= (unsigned)n_rates) return false;
    const fh_rate q = rates[r];
    if (q.up <= 0 || q.down <= 0 || q.n_taps < 0 || q.taps_off < 0 || (long long)q.taps_off + q.n_taps > bank_len) return false;
    out = {q.n_taps ? tap_bank + q.taps_off : nullptr, q.up, q.down, q.n_taps, q.n_pre_remove};
    return true;
  }
};

// out[i] = sum_j x[j] * h[(i + pre) * down - j * up],  h zero outside [0, n_taps)
template <class Loc, class Flt>
__global__ __launch_bounds__(256) void resample_poly_kernel(Loc loc, Flt flt) {
  fe_filter f;
  if (!flt(blockIdx.y, f)) return;
  const fh_clip c = loc(blockIdx.y);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c.len_out) return;
  if (Flt::kMayCopy && !f.h) {
    c.dst[i] = i < c.len_in ? c.src[i] : 0.f;
    return;
  }
  const long long pos = (long long)(i + f.pre) * f.down;
  long long j_hi = pos / f.up;
  if (j_hi > c.len_in - 1) j_hi = c.len_in - 1;
  float acc = 0.f;
  // ascending j == descending tap index; scipy's upfirdn walks the taps in ascending order,
  // so accumulate from the smallest tap index (largest j) down to match its summation order.
  for (long long j = j_hi; j >= 0; --j) {
    long long k = pos - j * f.up;
    if (k >= f.n_taps) break;
    acc = fmaf(c.src[j], f.h[k], acc);
  }
  c.dst[i] = acc;
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

int peak_abs_blocks(int len) {      // blocks along x of the two peak_abs entries: capped, the kernel strides
  const int bx = fh_cdiv(len, 256);
  return bx > 1024 ? 1024 : bx;
}

}  // namespace

#define FH_CHECK_CLIPS(name) \
  FH_CHECK_ARG(clips && n_clips > 0 && n_clips < 65536, name ": bad clip table (1 .. 65535 clips)")

extern "C" int fh_sizeof_clip(void) { return (int)sizeof(fh_clip); }
extern "C" int fh_sizeof_rate(void) { return (int)sizeof(fh_rate); }

extern "C" int fh_frame_f32(const float* audio, const float* window, float* frames, int batch,
                            int len, int n_frames, int nfft, int hop, int pad, int pad_mode,
                            void* stream) {
  FH_CHECK_ARG(audio && window && frames && batch > 0 && len > 0 && n_frames > 0 && nfft > 0 && hop > 0 && pad >= 0 &&
               (pad_mode == 0 || pad_mode == 1), "fh_frame_f32: bad args");
  FH_CHECK_ARG(pad_mode == 1 || pad < len, "fh_frame_f32: reflect pad %d needs len > pad", pad);
  FH_CHECK_ARG(hop * (n_frames - 1) + nfft <= len + 2 * pad, "fh_frame_f32: frames exceed padded signal");
  hipLaunchKernelGGL(frame_kernel<BatchedClips>, dim3(n_frames, batch), dim3(256), 0, (hipStream_t)stream,
                     BatchedClips{audio, nullptr, len, 0, n_frames}, window, frames, nfft, hop, pad, pad_mode);
  FH_CHECK_LAUNCH("fh_frame_f32");
  return FH_OK;
}

extern "C" int fh_frame_seg_f32(const fh_clip* clips, int n_clips, int max_rows, int min_len, const float* window,
                                float* frames, int nfft, int hop, int pad, int pad_mode, void* stream) {
  FH_CHECK_CLIPS("fh_frame_seg_f32");
  FH_CHECK_ARG(window && frames && max_rows > 0 && min_len > 0 && nfft > 0 && hop > 0 && pad >= 0 &&
               (pad_mode == 0 || pad_mode == 1), "fh_frame_seg_f32: bad args");
  FH_CHECK_ARG(pad_mode == 1 || pad < min_len, "fh_frame_seg_f32: reflect pad %d needs len > pad", pad);
  hipLaunchKernelGGL(frame_kernel<ClipTable>, dim3(max_rows, n_clips), dim3(256), 0, (hipStream_t)stream,
                     ClipTable{clips}, window, frames, nfft, hop, pad, pad_mode);
  FH_CHECK_LAUNCH("fh_frame_seg_f32");
  return FH_OK;
}

extern "C" int fh_spec_energy_f32(const float* spec, float* energy, int batch, int n_frames,
                                  void* stream) {
  FH_CHECK_ARG(spec && energy && batch > 0 && n_frames > 0, "fh_spec_energy_f32: bad args");
  hipLaunchKernelGGL(spec_energy_kernel<BatchedClips>, dim3(P_BLOCKS, batch), dim3(32 * SE_LANES), 0,
                     (hipStream_t)stream, batched_rows(n_frames), spec, energy);
  FH_CHECK_LAUNCH("fh_spec_energy_f32");
  return FH_OK;
}

extern "C" int fh_spec_energy_seg_f32(const float* spec, float* energy, const int32_t* seg, int n_seg, void* stream) {
  FH_CHECK_ARG(spec && energy && seg && n_seg > 0 && n_seg < 65536, "fh_spec_energy_seg_f32: bad args");
  hipLaunchKernelGGL(spec_energy_kernel<RowTable>, dim3(P_BLOCKS, n_seg), dim3(32 * SE_LANES), 0, (hipStream_t)stream,
                     RowTable{seg}, spec, energy);
  FH_CHECK_LAUNCH("fh_spec_energy_seg_f32");
  return FH_OK;
}

extern "C" int fh_cutoff_index_f32(const float* energy, int32_t* cr, int batch, int nbins, float thr,
                                   void* stream) {
  FH_CHECK_ARG(energy && cr && batch > 0 && nbins > 1 && nbins <= 1025, "fh_cutoff_index_f32: bad args");
  hipLaunchKernelGGL(cutoff_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, energy, cr, nbins, thr);
  FH_CHECK_LAUNCH("fh_cutoff_index_f32");
  return FH_OK;
}

extern "C" int fh_mel_energy_f32(const float* mel, float* energy, int batch, int n, int d, void* stream) {
  FH_CHECK_ARG(mel && energy && batch > 0 && n > 0 && d > 0, "fh_mel_energy_f32: bad args");
  hipLaunchKernelGGL(mel_energy_kernel<BatchedClips>, dim3(fh_cdiv(d, 256), batch), dim3(256), 0, (hipStream_t)stream,
                     batched_rows(n), mel, energy, d);
  FH_CHECK_LAUNCH("fh_mel_energy_f32");
  return FH_OK;
}

extern "C" int fh_mel_energy_seg_f32(const float* mel, float* energy, const int32_t* seg, int n_seg, int d,
                                     void* stream) {
  FH_CHECK_ARG(mel && energy && seg && n_seg > 0 && n_seg < 65536 && d > 0, "fh_mel_energy_seg_f32: bad args");
  hipLaunchKernelGGL(mel_energy_kernel<RowTable>, dim3(fh_cdiv(d, 256), n_seg), dim3(256), 0, (hipStream_t)stream,
                     RowTable{seg}, mel, energy, d);
  FH_CHECK_LAUNCH("fh_mel_energy_seg_f32");
  return FH_OK;
}

extern "C" int fh_mel_splice_f32(const float* low, const float* high, const int32_t* cut, float* out,
                                 int batch, int n, int d, void* stream) {
  FH_CHECK_ARG(low && high && cut && out && batch > 0 && n > 0 && d > 0, "fh_mel_splice_f32: bad args");
  hipLaunchKernelGGL(mel_splice_kernel<BatchedClips>, dim3(fh_cdiv((long long)n * d, 256), batch), dim3(256), 0,
                     (hipStream_t)stream, batched_rows(n), low, high, cut, out, d);
  FH_CHECK_LAUNCH("fh_mel_splice_f32");
  return FH_OK;
}

extern "C" int fh_mel_splice_seg_f32(const float* low, const float* high, const int32_t* cut, float* out,
                                     const int32_t* seg, int n_seg, int max_n, int d, void* stream) {
  FH_CHECK_ARG(low && high && cut && out && seg && n_seg > 0 && n_seg < 65536 && max_n > 0 && d > 0,
               "fh_mel_splice_seg_f32: bad args");
  hipLaunchKernelGGL(mel_splice_kernel<RowTable>, dim3(fh_cdiv((long long)max_n * d, 256), n_seg), dim3(256), 0,
                     (hipStream_t)stream, RowTable{seg}, low, high, cut, out, d);
  FH_CHECK_LAUNCH("fh_mel_splice_seg_f32");
  return FH_OK;
}

extern "C" int fh_axpby_f32(const float* x, float a, const float* y, float b, float* out, long long n,
                            void* stream) {
  FH_CHECK_ARG(x && y && out && n > 0, "fh_axpby_f32: bad args");
  hipLaunchKernelGGL(axpby_kernel, dim3(fh_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, a, y, b, out, n);
  FH_CHECK_LAUNCH("fh_axpby_f32");
  return FH_OK;
}

extern "C" int fh_spec_splice_f32(const float* pred, const float* src, const int32_t* cr, float* out,
                                  int batch, int n_frames, void* stream) {
  FH_CHECK_ARG(pred && src && cr && out && batch > 0 && n_frames > 0, "fh_spec_splice_f32: bad args");
  dim3 grid(fh_cdiv((long long)n_frames * P_WIDTH, 256), batch);
  hipLaunchKernelGGL(spec_splice_kernel<BatchedClips>, grid, dim3(256), 0, (hipStream_t)stream, batched_rows(n_frames),
                     pred, src, cr, out);
  FH_CHECK_LAUNCH("fh_spec_splice_f32");
  return FH_OK;
}

extern "C" int fh_spec_splice_seg_f32(const float* pred, const float* src, const int32_t* cr, float* out,
                                      const int32_t* seg, int n_seg, int max_rows, void* stream) {
  FH_CHECK_ARG(pred && src && cr && out && seg && n_seg > 0 && n_seg < 65536 && max_rows > 0,
               "fh_spec_splice_seg_f32: bad args");
  dim3 grid(fh_cdiv((long long)max_rows * P_WIDTH, 256), n_seg);
  hipLaunchKernelGGL(spec_splice_kernel<RowTable>, grid, dim3(256), 0, (hipStream_t)stream, RowTable{seg}, pred, src, cr,
                     out);
  FH_CHECK_LAUNCH("fh_spec_splice_seg_f32");
  return FH_OK;
}

extern "C" int fh_istft_ola_f32(const float* frames, const float* window, float* y,
                                uint32_t* peak_bits, int batch, int n_frames, int len, int nfft,
                                int hop, void* stream) {
  FH_CHECK_ARG(frames && window && y && peak_bits && batch > 0 && n_frames > 0 && len > 0 && nfft > 0 && hop > 0,
               "fh_istft_ola_f32: bad args");
  dim3 grid(fh_cdiv(len, 256), batch);
  hipLaunchKernelGGL(istft_ola_kernel<BatchedClips>, grid, dim3(256), 0, (hipStream_t)stream,
                     BatchedClips{nullptr, y, 0, len, n_frames}, frames, window, peak_bits, nfft, hop);
  FH_CHECK_LAUNCH("fh_istft_ola_f32");
  return FH_OK;
}

extern "C" int fh_istft_ola_seg_f32(const float* frames, const float* window, const fh_clip* clips, int n_clips,
                                    int max_len, uint32_t* peak_bits, int nfft, int hop, void* stream) {
  FH_CHECK_CLIPS("fh_istft_ola_seg_f32");
  FH_CHECK_ARG(frames && window && peak_bits && max_len > 0 && nfft > 0 && hop > 0, "fh_istft_ola_seg_f32: bad args");
  hipLaunchKernelGGL(istft_ola_kernel<ClipTable>, dim3(fh_cdiv(max_len, 256), n_clips), dim3(256), 0, (hipStream_t)stream,
                     ClipTable{clips}, frames, window, peak_bits, nfft, hop);
  FH_CHECK_LAUNCH("fh_istft_ola_seg_f32");
  return FH_OK;
}

extern "C" int fh_peak_abs_f32(const float* x, uint32_t* peak_bits, int batch, int len, void* stream) {
  FH_CHECK_ARG(x && peak_bits && batch > 0 && len > 0, "fh_peak_abs_f32: bad args");
  hipLaunchKernelGGL(peak_abs_kernel<BatchedClips>, dim3(peak_abs_blocks(len), batch), dim3(256), 0, (hipStream_t)stream,
                     BatchedClips{nullptr, const_cast<float*>(x), 0, len, 0}, peak_bits);
  FH_CHECK_LAUNCH("fh_peak_abs_f32");
  return FH_OK;
}

extern "C" int fh_peak_abs_seg_f32(const fh_clip* clips, int n_clips, int max_len, uint32_t* peak_bits, void* stream) {
  FH_CHECK_CLIPS("fh_peak_abs_seg_f32");
  FH_CHECK_ARG(peak_bits && max_len > 0, "fh_peak_abs_seg_f32: bad args");
  hipLaunchKernelGGL(peak_abs_kernel<ClipTable>, dim3(peak_abs_blocks(max_len), n_clips), dim3(256), 0,
                     (hipStream_t)stream, ClipTable{clips}, peak_bits);
  FH_CHECK_LAUNCH("fh_peak_abs_seg_f32");
  return FH_OK;
}

extern "C" int fh_peak_scale_f32(float* y, const uint32_t* peak_bits, int batch, int len,
                                 float target, void* stream) {
  FH_CHECK_ARG(y && peak_bits && batch > 0 && len > 0, "fh_peak_scale_f32: bad args");
  hipLaunchKernelGGL(peak_scale_kernel<BatchedClips>, dim3(fh_cdiv(len, 256), batch), dim3(256), 0, (hipStream_t)stream,
                     BatchedClips{nullptr, y, 0, len, 0}, peak_bits, target);
  FH_CHECK_LAUNCH("fh_peak_scale_f32");
  return FH_OK;
}

extern "C" int fh_peak_scale_seg_f32(const fh_clip* clips, int n_clips, int max_len, const uint32_t* peak_bits,
                                     float target, void* stream) {
  FH_CHECK_CLIPS("fh_peak_scale_seg_f32");
  FH_CHECK_ARG(peak_bits && max_len > 0, "fh_peak_scale_seg_f32: bad args");
  hipLaunchKernelGGL(peak_scale_kernel<ClipTable>, dim3(fh_cdiv(max_len, 256), n_clips), dim3(256), 0, (hipStream_t)stream,
                     ClipTable{clips}, peak_bits, target);
  FH_CHECK_LAUNCH("fh_peak_scale_seg_f32");
  return FH_OK;
}

extern "C" int fh_resample_poly_f32(const float* x, const float* taps, float* y, int batch,
                                    int len_in, int len_out, int up, int down, int n_taps,
                                    int n_pre_remove, void* stream) {
  FH_CHECK_ARG(x && taps && y && batch > 0 && len_in > 0 && len_out > 0 && up > 0 && down > 0, "fh_resample_poly_f32: bad args");
  hipLaunchKernelGGL((resample_poly_kernel<BatchedClips, LaunchFilter<false>>), dim3(fh_cdiv(len_out, 256), batch), dim3(256),
                     0, (hipStream_t)stream, BatchedClips{x, y, len_in, len_out, 0},
                     LaunchFilter<false>{{taps, up, down, n_taps, n_pre_remove}});
  FH_CHECK_LAUNCH("fh_resample_poly_f32");
  return FH_OK;
}

extern "C" int fh_resample_poly_seg_f32(const fh_clip* clips, int n_clips, int max_len_out, const float* taps, int up,
                                        int down, int n_taps, int n_pre_remove, void* stream) {
  FH_CHECK_CLIPS("fh_resample_poly_seg_f32");
  FH_CHECK_ARG(max_len_out > 0 && up > 0 && down > 0, "fh_resample_poly_seg_f32: bad args");
  FH_CHECK_ARG(taps ? n_taps > 0 : (up == 1 && down == 1), "fh_resample_poly_seg_f32: no taps for %d / %d", up, down);
  hipLaunchKernelGGL((resample_poly_kernel<ClipTable, LaunchFilter<true>>), dim3(fh_cdiv(max_len_out, 256), n_clips),
                     dim3(256), 0, (hipStream_t)stream, ClipTable{clips},
                     LaunchFilter<true>{{taps, up, down, n_taps, n_pre_remove}});
  FH_CHECK_LAUNCH("fh_resample_poly_seg_f32");
  return FH_OK;
}

extern "C" int fh_resample_poly_rates_seg_f32(const fh_clip* clips, const int32_t* rate_of, int n_clips, int max_len_out,
                                              const fh_rate* rates, int n_rates, const float* tap_bank, int bank_len,
                                              void* stream) {
  FH_CHECK_CLIPS("fh_resample_poly_rates_seg_f32");
  FH_CHECK_ARG(rate_of && rates && n_rates >= 1, "fh_resample_poly_rates_seg_f32: bad rate table (rate_of, rates, n_rates >= 1)");
  FH_CHECK_ARG(max_len_out > 0, "fh_resample_poly_rates_seg_f32: bad max_len_out %d", max_len_out);
  FH_CHECK_ARG(bank_len >= 0 && (tap_bank || bank_len == 0), "fh_resample_poly_rates_seg_f32: bad tap bank (%d floats)",
               bank_len);
  hipLaunchKernelGGL((resample_poly_kernel<ClipTable, RowFilter>), dim3(fh_cdiv(max_len_out, 256), n_clips), dim3(256), 0,
                     (hipStream_t)stream, ClipTable{clips}, RowFilter{rate_of, rates, n_rates, tap_bank, bank_len});
  FH_CHECK_LAUNCH("fh_resample_poly_rates_seg_f32");
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
