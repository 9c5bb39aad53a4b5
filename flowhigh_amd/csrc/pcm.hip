// The last step of delivery (FlowHighSR.generate*(pcm=, dither=, interleaved=)): float32 rows -> PCM on the device, quantised,
// optionally dithered, planar or interleaved.  flowhigh_amd/pcm.py is the definition; the kernel gives its bits.
//   fh_pcm_i16_f32, fh_pcm_s24_f32           n_clips clips of `channels` planar rows of `len` floats, back to back
//   fh_pcm_i16_seg_f32, fh_pcm_s24_seg_f32   a device table of clips, each with its own channels, len, source rows (pointer +
//                                            pitch) and destination
// in int16, or in 24 bits (pcm='s24': container 3, 3 bytes a sample at any byte address; pcm='s24in32': container 4, an int32).
// The four are the instantiations pcm_kernel<locator, format> of one kernel: it finds its clip, refuses what a device table may
// hold, and calls the encoder bodies of pcm_common.h, which the encoder of a stream's blocks (stream_delivery.hip) calls too.  So
// a clip gets the same bits from the batched and the segment entry.  Grid: (blocks of 256 runs, clip, channel).
#include "fh_common.h"
#include "pcm_common.h"
#include "philox.h"

namespace {

// One clip as the bodies see it: the source of pcm_common.h over rows a pitch apart.  Loads are two 16-byte reads where the
// run is whole and its first float 16-byte aligned, else eight 4-byte reads.
struct pcm_view {
  const float* src;        // row c at src + c * pitch
  unsigned char* dst;
  long long pitch;
  int C, T;
  __device__ int channels() const { return C; }
  __device__ int len() const { return T; }
  __device__ long long origin() const { return 0; }
  __device__ float at(int ch, long long t) const { return src[(long long)ch * pitch + t]; }
  __device__ void load_run(int ch, long long first, float (&x)[RUN]) const {
    const float* __restrict__ row = src + (long long)ch * pitch;
    if (first >= 0 && first + RUN <= T && (((size_t)(row + first)) & 15) == 0) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(row + first), b = *reinterpret_cast<const f32x4*>(row + first + 4);
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
      x[k] = (t >= 0 && t < T) ? row[t] : 0.f;
    }
  }
};

struct BatchedPcm {        // equal clips back to back, `size` bytes a sample: clip b is computed
  const float* x;
  unsigned char* y;
  int channels, len, size;
  __device__ pcm_view operator()(int b) const {
    const size_t per = (size_t)channels * len;
    return {x + b * per, y + b * per * size, (long long)len, channels, len};
  }
};
struct PcmTable {          // one fh_pcm_clip per clip on the device
  const fh_pcm_clip* clips;
  __device__ pcm_view operator()(int b) const {
    const fh_pcm_clip c = clips[b];
    return {c.src, reinterpret_cast<unsigned char*>(c.dst), (long long)c.pitch, c.channels, c.len};
  }
};

template <class Loc, class Fmt>
__global__ __launch_bounds__(PCM_THREADS) void pcm_kernel(Loc loc, Fmt fmt, const unsigned long long* __restrict__ keys,
                                                          int interleaved) {
  const pcm_view c = loc(blockIdx.y);
  const int ch = blockIdx.z;
  if (c.C < 1 || c.C > 8 || c.T < 1 || ch >= c.C || !fmt.ok(c.dst)) return;      // (a table lives on the device: checked)
  const unsigned long long* __restrict__ key = keys ? keys + 2 * blockIdx.y : nullptr;
  if (interleaved)
    encode_interleaved(fmt, c, ch, c.dst, key);
  else
    encode_row(fmt, c, ch, c.dst + (size_t)ch * c.T * fmt.size(), key);
}

template <class Loc, class Fmt>
void launch_pcm(Loc loc, Fmt fmt, int max_len, int n_clips, int max_channels, const uint64_t* keys, int interleaved, void* stream) {
  hipLaunchKernelGGL((pcm_kernel<Loc, Fmt>), dim3(pcm_blocks(max_len), n_clips, max_channels), dim3(PCM_THREADS), 0,
                     (hipStream_t)stream, loc, fmt, (const unsigned long long*)keys, interleaved ? 1 : 0);
}

}  // namespace

// The shape checks of the four entries (channels and len: the batched entry's own, the segment entry's largest)
#define FH_CHECK_PCM_CLIPS(name, channels, len)                                                       \
  FH_CHECK_ARG(n_clips > 0 && n_clips < 65536, name ": %d clips (1 .. 65535)", n_clips);              \
  FH_CHECK_ARG(channels >= 1 && channels <= 8, name ": %d channels (1 .. 8)", channels);              \
  FH_CHECK_ARG(len > 0, name ": " #len " %d must be positive", len)

extern "C" int fh_sizeof_pcm_clip(void) { return (int)sizeof(fh_pcm_clip); }

extern "C" int fh_pcm_i16_f32(const float* x, int16_t* y, const uint64_t* keys, int n_clips, int channels, int len,
                              int interleaved, void* stream) {
  FH_CHECK_ARG(x && y, "fh_pcm_i16_f32: null pointer (x %p, y %p)", (const void*)x, (void*)y);
  FH_CHECK_PCM_CLIPS("fh_pcm_i16_f32", channels, len);
  FH_CHECK_ARG((((size_t)x) & 3) == 0 && (((size_t)y) & 1) == 0, "fh_pcm_i16_f32: x must be 4-byte, y 2-byte aligned");
  launch_pcm(BatchedPcm{x, (unsigned char*)y, channels, len, 2}, I16{}, len, n_clips, channels, keys, interleaved, stream);
  FH_CHECK_LAUNCH("fh_pcm_i16_f32");
  return FH_OK;
}

extern "C" int fh_pcm_i16_seg_f32(const fh_pcm_clip* clips, int n_clips, int max_channels, int max_len, const uint64_t* keys,
                                  int interleaved, void* stream) {
  FH_CHECK_ARG(clips, "fh_pcm_i16_seg_f32: null clip table");
  FH_CHECK_PCM_CLIPS("fh_pcm_i16_seg_f32", max_channels, max_len);
  launch_pcm(PcmTable{clips}, I16{}, max_len, n_clips, max_channels, keys, interleaved, stream);
  FH_CHECK_LAUNCH("fh_pcm_i16_seg_f32");
  return FH_OK;
}

extern "C" int fh_pcm_s24_f32(const float* x, void* y, const uint64_t* keys, int n_clips, int channels, int len, int interleaved,
                              int container, void* stream) {
  FH_CHECK_ARG(x && y, "fh_pcm_s24_f32: null pointer (x %p, y %p)", (const void*)x, y);
  FH_CHECK_PCM_CLIPS("fh_pcm_s24_f32", channels, len);
  FH_CHECK_PCM_CONTAINER("fh_pcm_s24_f32");
  FH_CHECK_ARG((((size_t)x) & 3) == 0, "fh_pcm_s24_f32: x must be 4-byte aligned");
  FH_CHECK_ARG(container == 3 || (((size_t)y) & 3) == 0, "fh_pcm_s24_f32: an int32 y must be 4-byte aligned");
  launch_pcm(BatchedPcm{x, (unsigned char*)y, channels, len, container}, S24{container}, len, n_clips, channels, keys, interleaved,
             stream);
  FH_CHECK_LAUNCH("fh_pcm_s24_f32");
  return FH_OK;
}

extern "C" int fh_pcm_s24_seg_f32(const fh_pcm_clip* clips, int n_clips, int max_channels, int max_len, const uint64_t* keys,
                                  int interleaved, int container, void* stream) {
  FH_CHECK_ARG(clips, "fh_pcm_s24_seg_f32: null clip table");
  FH_CHECK_PCM_CLIPS("fh_pcm_s24_seg_f32", max_channels, max_len);
  FH_CHECK_PCM_CONTAINER("fh_pcm_s24_seg_f32");
  launch_pcm(PcmTable{clips}, S24{container}, max_len, n_clips, max_channels, keys, interleaved, stream);
  FH_CHECK_LAUNCH("fh_pcm_s24_seg_f32");
  return FH_OK;
}
