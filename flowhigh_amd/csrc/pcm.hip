// The last step of delivery (FlowHighSR.generate*(pcm='int16', dither=, interleaved=)): float32 rows -> int16 PCM on the device,
// quantised, optionally dithered, planar or interleaved.  flowhigh_amd/pcm.py is the definition; the kernel gives its bits.
//   fh_pcm_i16_f32       n_clips clips of `channels` planar rows of `len` floats, back to back
//   fh_pcm_i16_seg_f32   a device table of clips, each with its own channels, len, source rows (pointer + pitch) and destination
// Both are instantiations of one kernel body that differ in the clip locator, so a clip gets the same bits from either.
//   sample x -> v = fl(x * 32768) [exact] -> v = fl(v + d) when dithering -> rint (ties to even) -> clamp to [-32768, 32767];
//   NaN -> 0.
//   d of (channel c, sample t) under the clip's key (seed, stream): Philox4x32-10 of the counter (t >> 1, stream) under the key
//   (seed.lo ^ 'PCM1', seed.hi ^ c); even t takes (r0, r1), odd t (r2, r3); d = ((ra >> 8) - (rb >> 8)) 2^-24: triangular on
//   (-1, 1) LSB, exact in fp32.  It depends on (key, c, t) only -- not on the batch, the layout or the number of channels.
// Grid: (blocks of 256 runs, clip, channel).  A thread owns a run of 8 consecutive samples of one channel.  Planar output: run s
// is the 16-byte word s of the row's memory counted from the aligned address at or below the row (as level.hip's row gain),
// so a run wholly inside the row is one 16-byte store and the (at most two) runs over an end go element by element.  Interleaved
// output: runs start at the row's first sample.  With C = 2, 4 or 8 and the clip's destination aligned to a frame (2 C bytes) the
// blocks of channel 0 encode every channel and store each sample frame as one 4-, 8- or 16-byte word (pcm_frames); otherwise
// every sample is a 2-byte store at its place in its frame.  Loads are two 16-byte reads where the run's first float is 16-byte
// aligned, else eight 4-byte reads.  Which stores are used never changes a value.
// encode() and dither_run() are in pcm_common.h: the encoder of a stream's blocks (stream_delivery.hip) uses the same two.
//   fh_pcm_s24_f32, fh_pcm_s24_seg_f32   the same two forms in 24 bits (pcm='s24': 3 bytes a sample at any byte address,
//                        pcm='s24in32': an int32): pcm_s24_kernel below; encode24() and the stores of a run are in pcm_common.h
#include "fh_common.h"
#include "pcm_common.h"
#include "philox.h"

namespace {

struct pcm_view {          // one clip as the kernel body sees it
  const float* src;        // row c at src + c * pitch
  int16_t* dst;
  long long pitch;
  int channels, len;
};

struct BatchedPcm {        // equal clips back to back: clip b is computed
  const float* x;
  int16_t* y;
  int channels, len;
  __device__ pcm_view operator()(int b) const {
    const size_t per = (size_t)channels * len;
    return {x + b * per, y + b * per, (long long)len, channels, len};
  }
};
struct PcmTable {          // one fh_pcm_clip per clip on the device
  const fh_pcm_clip* clips;
  __device__ pcm_view operator()(int b) const {
    const fh_pcm_clip c = clips[b];
    return {c.src, c.dst, (long long)c.pitch, c.channels, c.len};
  }
};

// x[k] = sample first + k of the row at src, 0 outside [0, len): two 16-byte reads where the run is whole and aligned
__device__ __forceinline__ void load_run(const float* __restrict__ src, long long first, int len, bool whole, float (&x)[RUN]) {
  if (whole && (((size_t)(src + first)) & 15) == 0) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + first), b = *reinterpret_cast<const f32x4*>(src + first + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[k] = a[k];
      x[4 + k] = b[k];
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    const long long t = first + k;
    x[k] = (t >= 0 && t < len) ? src[t] : 0.f;
  }
}

// Interleaved output of a clip of C = 2, 4 or 8 channels whose destination is aligned to a frame (2 C bytes): the thread encodes
// its run of every channel and stores each sample frame as ONE 4-, 8- or 16-byte word.
template <int C>
__device__ __forceinline__ void pcm_frames(const pcm_view& c, const unsigned long long* __restrict__ keys) {
  typedef short frame_t __attribute__((ext_vector_type(C)));
  const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * RUN;
  if (first >= c.len) return;
  const bool whole = first + RUN <= c.len;
  unsigned long long seed = 0, strm = 0;
  if (keys) {
    seed = keys[2 * blockIdx.y];
    strm = keys[2 * blockIdx.y + 1];
  }
  frame_t o[RUN];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    float x[RUN], d[RUN];
    load_run(c.src + (long long)ch * c.pitch, first, c.len, whole, x);
#pragma unroll
    for (int k = 0; k < RUN; ++k) d[k] = 0.f;
    if (keys) dither_run(seed, strm, ch, first, d);
#pragma unroll
    for (int k = 0; k < RUN; ++k) o[k][ch] = encode(x[k], d[k]);
  }
  frame_t* __restrict__ frames = reinterpret_cast<frame_t*>(c.dst);
#pragma unroll
  for (int k = 0; k < RUN; ++k)
    if (first + k < c.len) frames[first + k] = o[k];
}

template <class Loc>
__global__ __launch_bounds__(256) void pcm_i16_kernel(Loc loc, const unsigned long long* __restrict__ keys, int interleaved) {
  const pcm_view c = loc(blockIdx.y);
  const int ch = blockIdx.z;
  if (c.channels < 1 || c.channels > 8 || c.len < 1 || ch >= c.channels) return;      // (a table lives on the device: checked)
  if (interleaved && (c.channels == 2 || c.channels == 4 || c.channels == 8) && ((size_t)c.dst & (2 * c.channels - 1)) == 0) {
    if (ch != 0) return;                        // (the blocks of channel 0 write whole frames)
    if (c.channels == 2)
      pcm_frames<2>(c, keys);
    else if (c.channels == 4)
      pcm_frames<4>(c, keys);
    else
      pcm_frames<8>(c, keys);
    return;
  }
  const float* __restrict__ src = c.src + (long long)ch * c.pitch;
  int16_t* __restrict__ row = interleaved ? c.dst : c.dst + (size_t)ch * c.len;
  const int lead = interleaved ? 0 : (int)(((size_t)row >> 1) & (RUN - 1));      // elements between the aligned address and the row
  const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * RUN - lead;   // the run's first sample
  if (first >= c.len) return;
  const bool whole = first >= 0 && first + RUN <= c.len;

  float x[RUN], d[RUN];
  load_run(src, first, c.len, whole, x);
#pragma unroll
  for (int k = 0; k < RUN; ++k) d[k] = 0.f;
  if (keys) dither_run(keys[2 * blockIdx.y], keys[2 * blockIdx.y + 1], ch, first, d);

  if (whole && !interleaved) {
    i16x8 o;
#pragma unroll
    for (int k = 0; k < RUN; ++k) o[k] = encode(x[k], d[k]);
    *reinterpret_cast<i16x8*>(row + first) = o;
    return;
  }
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    const long long t = first + k;
    if (t < 0 || t >= c.len) continue;
    const short o = encode(x[k], d[k]);
    if (interleaved)
      row[(size_t)t * c.channels + ch] = o;
    else
      row[t] = o;
  }
}

int pcm_blocks(int len) { return fh_cdiv(((long long)len + RUN - 1) / RUN + 1, 256); }      // runs of a row at any alignment

// ---- 24 bits: pcm='s24' (container 3: packed, 3 bytes a sample) and 's24in32' (container 4: int32) ---------------------------
// The locators of the int16 kernel with dst as a byte address.
struct pcm24_view {
  const float* src;
  unsigned char* dst;
  long long pitch;
  int channels, len;
};
struct BatchedPcm24 {
  const float* x;
  unsigned char* y;
  int channels, len, container;
  __device__ pcm24_view operator()(int b) const {
    const size_t per = (size_t)channels * len;
    return {x + b * per, y + b * per * container, (long long)len, channels, len};
  }
};
struct PcmTable24 {
  const fh_pcm_clip* clips;
  __device__ pcm24_view operator()(int b) const {
    const fh_pcm_clip c = clips[b];
    return {c.src, reinterpret_cast<unsigned char*>(c.dst), (long long)c.pitch, c.channels, c.len};
  }
};

// Grid as pcm_i16_kernel's.  Planar: the blocks of channel ch own the row of that channel, N = len samples.  Interleaved: the
// clip is ONE flat row of N = len * C samples, flat sample s = sample s / C of channel s % C, and the blocks (x, z) with z < C
// share its runs: run (z * gridDim.x + x) * 256 + thread (C * gridDim.x * 256 >= C * (ceil(len / 8) + 1) runs, enough at any
// alignment); a run's 8 samples lie in up to 8 channels, so each takes its own Philox block (dither_at).  Every C takes that
// path.  The stores are store_run24's (pcm_common.h) either way; which ones are used never changes a value.
template <class Loc>
__global__ __launch_bounds__(256) void pcm_s24_kernel(Loc loc, const unsigned long long* __restrict__ keys, int interleaved,
                                                      int container) {
  const pcm24_view c = loc(blockIdx.y);
  const int ch = blockIdx.z;
  if (c.channels < 1 || c.channels > 8 || c.len < 1 || ch >= c.channels) return;      // (a table lives on the device: checked)
  if (container == 4 && ((size_t)c.dst & 3)) return;                                  // (the batched entry refused it already)
  unsigned long long seed = 0, strm = 0;
  if (keys) {
    seed = keys[2 * blockIdx.y];
    strm = keys[2 * blockIdx.y + 1];
  }
  int q[RUN];
  if (!interleaved) {
    unsigned char* __restrict__ row = c.dst + (size_t)ch * c.len * container;
    const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * RUN - lead24(row, container);
    if (first >= c.len) return;
    float x[RUN], d[RUN];
    load_run(c.src + (long long)ch * c.pitch, first, c.len, first >= 0 && first + RUN <= c.len, x);
#pragma unroll
    for (int k = 0; k < RUN; ++k) d[k] = 0.f;
    if (keys) dither_run(seed, strm, ch, first, d);
#pragma unroll
    for (int k = 0; k < RUN; ++k) q[k] = encode24(x[k], d[k]);
    store_run24(row, first, c.len, q, container);
    return;
  }
  const long long N = (long long)c.len * c.channels;
  const long long first = (((long long)ch * gridDim.x + blockIdx.x) * 256 + threadIdx.x) * RUN - lead24(c.dst, container);
  if (first >= N) return;
  const long long s0 = first < 0 ? 0 : first;
  long long t = N <= 0xFFFFFFFFll ? (long long)((unsigned)s0 / (unsigned)c.channels) : s0 / c.channels;
  int cc = (int)(s0 - t * c.channels);
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    const long long s = first + k;
    q[k] = 0;
    if (s < 0 || s >= N) continue;
    q[k] = encode24(c.src[(long long)cc * c.pitch + t], keys ? dither_at(seed, strm, cc, t) : 0.f);
    if (++cc == c.channels) {
      cc = 0;
      ++t;
    }
  }
  store_run24(c.dst, first, N, q, container);
}

}  // namespace

extern "C" int fh_sizeof_pcm_clip(void) { return (int)sizeof(fh_pcm_clip); }

extern "C" int fh_pcm_i16_f32(const float* x, int16_t* y, const uint64_t* keys, int n_clips, int channels, int len,
                              int interleaved, void* stream) {
  FH_CHECK_ARG(x && y, "fh_pcm_i16_f32: null pointer (x %p, y %p)", (const void*)x, (void*)y);
  FH_CHECK_ARG(n_clips > 0 && n_clips < 65536, "fh_pcm_i16_f32: %d clips (1 .. 65535)", n_clips);
  FH_CHECK_ARG(channels >= 1 && channels <= 8, "fh_pcm_i16_f32: %d channels (1 .. 8)", channels);
  FH_CHECK_ARG(len > 0, "fh_pcm_i16_f32: len %d must be positive", len);
  FH_CHECK_ARG((((size_t)x) & 3) == 0 && (((size_t)y) & 1) == 0, "fh_pcm_i16_f32: x must be 4-byte, y 2-byte aligned");
  hipLaunchKernelGGL(pcm_i16_kernel<BatchedPcm>, dim3(pcm_blocks(len), n_clips, channels), dim3(256), 0, (hipStream_t)stream,
                     BatchedPcm{x, y, channels, len}, (const unsigned long long*)keys, interleaved ? 1 : 0);
  FH_CHECK_LAUNCH("fh_pcm_i16_f32");
  return FH_OK;
}

extern "C" int fh_pcm_i16_seg_f32(const fh_pcm_clip* clips, int n_clips, int max_channels, int max_len, const uint64_t* keys,
                                  int interleaved, void* stream) {
  FH_CHECK_ARG(clips, "fh_pcm_i16_seg_f32: null clip table");
  FH_CHECK_ARG(n_clips > 0 && n_clips < 65536, "fh_pcm_i16_seg_f32: %d clips (1 .. 65535)", n_clips);
  FH_CHECK_ARG(max_channels >= 1 && max_channels <= 8, "fh_pcm_i16_seg_f32: %d channels (1 .. 8)", max_channels);
  FH_CHECK_ARG(max_len > 0, "fh_pcm_i16_seg_f32: max_len %d must be positive", max_len);
  hipLaunchKernelGGL(pcm_i16_kernel<PcmTable>, dim3(pcm_blocks(max_len), n_clips, max_channels), dim3(256), 0,
                     (hipStream_t)stream, PcmTable{clips}, (const unsigned long long*)keys, interleaved ? 1 : 0);
  FH_CHECK_LAUNCH("fh_pcm_i16_seg_f32");
  return FH_OK;
}

extern "C" int fh_pcm_s24_f32(const float* x, void* y, const uint64_t* keys, int n_clips, int channels, int len, int interleaved,
                              int container, void* stream) {
  FH_CHECK_ARG(x && y, "fh_pcm_s24_f32: null pointer (x %p, y %p)", (const void*)x, y);
  FH_CHECK_ARG(n_clips > 0 && n_clips < 65536, "fh_pcm_s24_f32: %d clips (1 .. 65535)", n_clips);
  FH_CHECK_ARG(channels >= 1 && channels <= 8, "fh_pcm_s24_f32: %d channels (1 .. 8)", channels);
  FH_CHECK_ARG(len > 0, "fh_pcm_s24_f32: len %d must be positive", len);
  FH_CHECK_ARG(container == 3 || container == 4, "fh_pcm_s24_f32: container %d (3: packed bytes, 4: int32)", container);
  FH_CHECK_ARG((((size_t)x) & 3) == 0, "fh_pcm_s24_f32: x must be 4-byte aligned");
  FH_CHECK_ARG(container == 3 || (((size_t)y) & 3) == 0, "fh_pcm_s24_f32: an int32 y must be 4-byte aligned");
  hipLaunchKernelGGL(pcm_s24_kernel<BatchedPcm24>, dim3(pcm_blocks(len), n_clips, channels), dim3(256), 0, (hipStream_t)stream,
                     BatchedPcm24{x, (unsigned char*)y, channels, len, container}, (const unsigned long long*)keys,
                     interleaved ? 1 : 0, container);
  FH_CHECK_LAUNCH("fh_pcm_s24_f32");
  return FH_OK;
}

extern "C" int fh_pcm_s24_seg_f32(const fh_pcm_clip* clips, int n_clips, int max_channels, int max_len, const uint64_t* keys,
                                  int interleaved, int container, void* stream) {
  FH_CHECK_ARG(clips, "fh_pcm_s24_seg_f32: null clip table");
  FH_CHECK_ARG(n_clips > 0 && n_clips < 65536, "fh_pcm_s24_seg_f32: %d clips (1 .. 65535)", n_clips);
  FH_CHECK_ARG(max_channels >= 1 && max_channels <= 8, "fh_pcm_s24_seg_f32: %d channels (1 .. 8)", max_channels);
  FH_CHECK_ARG(max_len > 0, "fh_pcm_s24_seg_f32: max_len %d must be positive", max_len);
  FH_CHECK_ARG(container == 3 || container == 4, "fh_pcm_s24_seg_f32: container %d (3: packed bytes, 4: int32)", container);
  hipLaunchKernelGGL(pcm_s24_kernel<PcmTable24>, dim3(pcm_blocks(max_len), n_clips, max_channels), dim3(256), 0,
                     (hipStream_t)stream, PcmTable24{clips}, (const unsigned long long*)keys, interleaved ? 1 : 0, container);
  FH_CHECK_LAUNCH("fh_pcm_s24_seg_f32");
  return FH_OK;
}
