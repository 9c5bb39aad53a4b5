// The PCM encoders, stated once for clips (pcm.hip) and for the blocks of a stream (stream_delivery.hip), in int16 and in 24 bits.
// flowhigh_amd/pcm.py is the definition.  A kernel locates its clip or group, refuses what it must, and calls one of four bodies:
//   encode_row        a planar row, runs aligned to the row's memory           (every format)
//   encode_frames<C>  interleaved int16, C = 2, 4, 8 at a frame-aligned address: one store per sample frame
//   encode_scattered  interleaved int16 otherwise: a 2-byte store at the sample's place in its frame
//   encode_flat       interleaved 24 bits: the clip as ONE flat row of len * C samples
// over two things the kernel hands them.  A source `Src` says where a sample comes from: channels(), len() (outputs per channel),
// load_run(ch, first, x) (samples first .. first + 7 of channel ch, 0 outside [0, len)), at(ch, t), and origin(), the absolute
// index of output 0 for the dither (a clip: 0; a stream's block: the job's `first`).  A format `Fmt` (I16, S24) says what a sample
// becomes and how a run of 8 codes is stored: code(x, d), ok(address), size(), lead(row), store_run(row, first, N, q).  The format
// is a template parameter of the kernels, so the 24-bit launches do not pay for the registers of encode_frames<8>.
// Which body and which store is used never changes a value: a clip has the same bits from the batched and the segment entry, and
// a stream's blocks add up to the one-shot bits.
#pragma once
#include "fh_common.h"
#include "philox.h"

namespace {

constexpr int RUN = 8;                          // samples per thread = one 16-byte store of int16
constexpr int PCM_THREADS = 256;                // threads of an encoder block: grid.x = pcm_blocks(len) blocks of them
constexpr unsigned KEY_TAG = 0x50434D31u;       // 'PCM1': keeps the dither's blocks apart from the prior's under the same key

inline int pcm_blocks(int len) { return fh_cdiv(((long long)len + RUN - 1) / RUN + 1, PCM_THREADS); }      // runs of a row at any alignment

#define FH_CHECK_PCM_CONTAINER(name) \
  FH_CHECK_ARG(container == 3 || container == 4, name ": container %d (3: packed bytes, 4: int32)", container)

typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- the samples -----------------------------------------------------------------------------------------------------------
// int16: v = fl(x * 32768) [exact] -> v = fl(v + d) -> rint (ties to even) -> clamp to [-32768, 32767]; NaN -> 0.
__device__ __forceinline__ short encode(float x, float d) {
  float v = __fmul_rn(x, 32768.f);
  v = __fadd_rn(v, d);
  float q = rintf(v);
  q = fminf(fmaxf(q, -32768.f), 32767.f);
  return (v != v) ? (short)0 : (short)(int)q;
}

// The 24-bit sample: v = x * 2^23 in float64 (exact, so contraction cannot change it), ONE float64 add of the dither (a float32
// add would round it away: x * 2^23 fills the float32 significand), rint to even, clamp to [-2^23, 2^23 - 1]; NaN -> 0.
__device__ __forceinline__ int encode24(float x, float d) {
  double v = __dmul_rn((double)x, 8388608.0);
  v = __dadd_rn(v, (double)d);
  double q = rint(v);
  q = fmin(fmax(q, -8388608.0), 8388607.0);
  return (v != v) ? 0 : (int)q;
}

// ---- the dither ------------------------------------------------------------------------------------------------------------
// d of (channel c, sample t) under the key (seed, stream): Philox4x32-10 of the counter (t >> 1, stream) under the key
// (seed.lo ^ 'PCM1', seed.hi ^ c); even t takes (r0, r1), odd t (r2, r3); d = ((ra >> 8) - (rb >> 8)) 2^-24: triangular on
// (-1, 1) LSB, exact in fp32.  It depends on (key, c, t) only -- not on the batch, the layout or the number of channels.
// d[k] = the dither of sample first + k of channel ch.  A run of 8 samples touches 4 Philox blocks when it starts on an even
// sample, 5 when on an odd one; with first < 0 the run's samples before t = 0 are never stored.
__device__ __forceinline__ void dither_run(unsigned long long seed, unsigned long long strm, int ch, long long first,
                                           float (&d)[RUN]) {
  const unsigned k0 = (unsigned)seed ^ KEY_TAG, k1 = (unsigned)(seed >> 32) ^ (unsigned)ch;
  const long long t0 = first < 0 ? 0 : first;
  const long long q0 = t0 >> 1;
  u32x4 r[RUN / 2 + 1];
#pragma unroll
  for (int j = 0; j <= RUN / 2; ++j) {
    const unsigned long long q = (unsigned long long)(q0 + j);
    if (j < RUN / 2 || (first & 1))
      r[j] = philox4x32_10(u32x4{(unsigned)q, (unsigned)(q >> 32), (unsigned)strm, (unsigned)(strm >> 32)}, k0, k1);
    else
      r[j] = u32x4{0u, 0u, 0u, 0u};
  }
  const int odd = (int)(first & 1);            // (first may be negative: & 1 is its parity all the same)
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    const long long t = first + k;              // sample t lies in block (t >> 1) - q0
    const int j = (int)((t >> 1) - q0);
    u32x4 rr = r[0];
#pragma unroll
    for (int m = 1; m <= RUN / 2; ++m) rr = (j == m) ? r[m] : rr;
    const bool hi = ((k + odd) & 1) != 0;
    const unsigned ra = hi ? rr[2] : rr[0], rb = hi ? rr[3] : rr[1];
    d[k] = (float)((int)(ra >> 8) - (int)(rb >> 8)) * 0x1p-24f;
  }
}

// The dither of ONE sample t >= 0 of channel ch: dither_run's value for it (one Philox block per sample; encode_flat, whose 8
// samples lie in up to 8 channels).
__device__ __forceinline__ float dither_at(unsigned long long seed, unsigned long long strm, int ch, long long t) {
  const unsigned k0 = (unsigned)seed ^ KEY_TAG, k1 = (unsigned)(seed >> 32) ^ (unsigned)ch;
  const unsigned long long q = (unsigned long long)t >> 1;
  const u32x4 r = philox4x32_10(u32x4{(unsigned)q, (unsigned)(q >> 32), (unsigned)strm, (unsigned)(strm >> 32)}, k0, k1);
  const bool hi = (t & 1) != 0;
  const unsigned ra = hi ? r[2] : r[0], rb = hi ? r[3] : r[1];
  return (float)((int)(ra >> 8) - (int)(rb >> 8)) * 0x1p-24f;
}

// x[k], d[k] = sample first + k of channel ch and its dither under the key (0 without one)
template <class Src>
__device__ __forceinline__ void sample_run(const Src& src, const unsigned long long* __restrict__ key, int ch, long long first,
                                           float (&x)[RUN], float (&d)[RUN]) {
  src.load_run(ch, first, x);
#pragma unroll
  for (int k = 0; k < RUN; ++k) d[k] = 0.f;
  if (key) dither_run(key[0], key[1], ch, src.origin() + first, d);
}

// ---- the formats -----------------------------------------------------------------------------------------------------------
// A row is N samples of size() bytes from the byte address `row` on.  A thread owns a run of 8 samples; run r starts at sample
// 8 r - lead(row), which puts every run of the row at an aligned address.  A run wholly inside the row goes out in wide stores,
// the at most two runs over a row end element by element.  Nothing outside [row, row + size() * N) is read or written, and no
// word is shared: neighbours that abut at any address the format takes stay intact.
struct I16 {                                    // int16: a run is 16 bytes, lead = the elements between the 16-byte grid and the row
  typedef short code_t;
  __device__ static short code(float x, float d) { return encode(x, d); }
  __device__ static bool ok(const void* p) { return ((size_t)p & 1) == 0; }
  __device__ static int size() { return 2; }
  __device__ static int lead(const unsigned char* row) { return (int)(((size_t)row >> 1) & (RUN - 1)); }
  __device__ static void store_run(unsigned char* __restrict__ row, long long first, long long N, const short (&q)[RUN]) {
    short* __restrict__ out = reinterpret_cast<short*>(row);
    if (first >= 0 && first + RUN <= N) {
      *reinterpret_cast<i16x8*>(out + first) = i16x8{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
      return;
    }
#pragma unroll
    for (int k = 0; k < RUN; ++k)
      if (first + k >= 0 && first + k < N) out[first + k] = q[k];
  }
};

// 24 bits in `container` bytes (3: the low three bytes, least significant first, at any byte address; 4: the int32, 4-byte
// aligned).  A run is 24 or 32 contiguous bytes, and lead puts it at an 8-byte (packed) or 32-byte (int32) boundary: 3 lead =
// row (mod 8) has the solution lead = 3 row, and 24 is a multiple of 8, so every run of the row is aligned alike.  A whole run
// is three 8-byte stores (two 16-byte ones for int32); the others go byte by byte (sample by sample for int32).
__device__ __forceinline__ void store_run24(unsigned char* __restrict__ row, long long first, long long N, const int (&q)[RUN],
                                            int container) {
  const bool whole = first >= 0 && first + RUN <= N;
  if (container == 4) {
    int* __restrict__ out = reinterpret_cast<int*>(row);
    if (whole) {
      *reinterpret_cast<i32x4*>(out + first) = i32x4{q[0], q[1], q[2], q[3]};
      *reinterpret_cast<i32x4*>(out + first + 4) = i32x4{q[4], q[5], q[6], q[7]};
      return;
    }
#pragma unroll
    for (int k = 0; k < RUN; ++k)
      if (first + k >= 0 && first + k < N) out[first + k] = q[k];
    return;
  }
  if (whole) {
    unsigned w[6];
#pragma unroll
    for (int h = 0; h < 2; ++h) {             // 4 samples = 12 bytes = 3 words
      const unsigned a = (unsigned)q[4 * h] & 0xFFFFFFu, b = (unsigned)q[4 * h + 1] & 0xFFFFFFu,
                     c = (unsigned)q[4 * h + 2] & 0xFFFFFFu, e = (unsigned)q[4 * h + 3] & 0xFFFFFFu;
      w[3 * h] = a | (b << 24);
      w[3 * h + 1] = (b >> 8) | (c << 16);
      w[3 * h + 2] = (c >> 16) | (e << 8);
    }
    u32x2* __restrict__ out = reinterpret_cast<u32x2*>(row + 3 * first);
    out[0] = u32x2{w[0], w[1]};
    out[1] = u32x2{w[2], w[3]};
    out[2] = u32x2{w[4], w[5]};
    return;
  }
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    const long long s = first + k;
    if (s < 0 || s >= N) continue;
    const unsigned u = (unsigned)q[k];
    row[3 * s] = (unsigned char)u;
    row[3 * s + 1] = (unsigned char)(u >> 8);
    row[3 * s + 2] = (unsigned char)(u >> 16);
  }
}

struct S24 {
  typedef int code_t;
  int container;
  __device__ static int code(float x, float d) { return encode24(x, d); }
  __device__ bool ok(const void* p) const { return container == 3 || ((size_t)p & 3) == 0; }
  __device__ int size() const { return container; }
  __device__ int lead(const unsigned char* row) const {
    return container == 3 ? (int)((3 * ((size_t)row & 7)) & 7) : (int)(((size_t)row >> 2) & (RUN - 1));
  }
  __device__ void store_run(unsigned char* __restrict__ row, long long first, long long N, const int (&q)[RUN]) const {
    store_run24(row, first, N, q, container);
  }
};

// ---- the four bodies.  Grid: x = blocks of 256 runs; ch = the block's channel --------------------------------------------
// The planar row of channel ch at `row`: run s is the s-th aligned run of the row's memory counted from the aligned address at
// or below the row, so a run wholly inside the row is stored whole.
template <class Fmt, class Src>
__device__ __forceinline__ void encode_row(const Fmt& fmt, const Src& src, int ch, unsigned char* __restrict__ row,
                                           const unsigned long long* __restrict__ key) {
  const int len = src.len();
  const long long first = ((long long)blockIdx.x * PCM_THREADS + threadIdx.x) * RUN - fmt.lead(row);      // the run's first sample
  if (len < 1 || first >= len) return;
  float x[RUN], d[RUN];
  sample_run(src, key, ch, first, x, d);
  typename Fmt::code_t q[RUN];
#pragma unroll
  for (int k = 0; k < RUN; ++k) q[k] = Fmt::code(x[k], d[k]);
  fmt.store_run(row, first, len, q);
}

// Interleaved int16 of C = 2, 4 or 8 channels at a destination aligned to a frame (2 C bytes): the thread encodes its run of
// every channel and stores each sample frame as ONE 4-, 8- or 16-byte word.  Runs start at the row's first sample.
template <int C, class Src>
__device__ __forceinline__ void encode_frames(const Src& src, unsigned char* __restrict__ dst,
                                              const unsigned long long* __restrict__ key) {
  typedef short frame_t __attribute__((ext_vector_type(C)));
  const int len = src.len();
  const long long first = ((long long)blockIdx.x * PCM_THREADS + threadIdx.x) * RUN;
  if (first >= len) return;
  frame_t o[RUN];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    float x[RUN], d[RUN];
    sample_run(src, key, ch, first, x, d);
#pragma unroll
    for (int k = 0; k < RUN; ++k) o[k][ch] = encode(x[k], d[k]);
  }
  frame_t* __restrict__ frames = reinterpret_cast<frame_t*>(dst);
#pragma unroll
  for (int k = 0; k < RUN; ++k)
    if (first + k < len) frames[first + k] = o[k];
}

// Interleaved int16 at any other channel count or address: every sample is a 2-byte store at its place in its frame.
template <class Src>
__device__ __forceinline__ void encode_scattered(const Src& src, int ch, unsigned char* __restrict__ dst,
                                                 const unsigned long long* __restrict__ key) {
  const int len = src.len(), C = src.channels();
  const long long first = ((long long)blockIdx.x * PCM_THREADS + threadIdx.x) * RUN;
  if (first >= len) return;
  float x[RUN], d[RUN];
  sample_run(src, key, ch, first, x, d);
  short* __restrict__ out = reinterpret_cast<short*>(dst);
#pragma unroll
  for (int k = 0; k < RUN; ++k)
    if (first + k < len) out[(size_t)(first + k) * C + ch] = encode(x[k], d[k]);
}

// Interleaved, as ONE flat row of N = len * C samples at dst: flat sample s is sample s / C of channel s % C, and the blocks
// (x, ch) with ch < C share its runs: run (ch * gridDim.x + x) * 256 + thread (C * gridDim.x * 256 >= C * (ceil(len / 8) + 1)
// runs, enough at any alignment).  A run's 8 samples lie in up to 8 channels, so each takes its own Philox block (dither_at).
template <class Fmt, class Src>
__device__ __forceinline__ void encode_flat(const Fmt& fmt, const Src& src, int ch, unsigned char* __restrict__ dst,
                                            const unsigned long long* __restrict__ key) {
  const int C = src.channels();
  const long long N = (long long)src.len() * C, origin = src.origin();
  const long long first = (((long long)ch * gridDim.x + blockIdx.x) * PCM_THREADS + threadIdx.x) * RUN - fmt.lead(dst);
  if (N < 1 || first >= N) return;
  const long long s0 = first < 0 ? 0 : first;
  long long t = N <= 0xFFFFFFFFll ? (long long)((unsigned)s0 / (unsigned)C) : s0 / C;      // (a 32-bit division where it can be)
  int cc = (int)(s0 - t * C);
  unsigned long long seed = 0, strm = 0;
  if (key) {
    seed = key[0];
    strm = key[1];
  }
  typename Fmt::code_t q[RUN];
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    const long long s = first + k;
    q[k] = 0;
    if (s < 0 || s >= N) continue;
    q[k] = Fmt::code(src.at(cc, t), key ? dither_at(seed, strm, cc, origin + t) : 0.f);
    if (++cc == C) {
      cc = 0;
      ++t;
    }
  }
  fmt.store_run(dst, first, N, q);
}

// The interleaved output of a format: int16 in whole frames where it can be (the blocks of channel 0 write them for the clip),
// else scattered; 24 bits flat at every channel count.
template <class Src>
__device__ __forceinline__ void encode_interleaved(const I16&, const Src& src, int ch, unsigned char* __restrict__ dst,
                                                   const unsigned long long* __restrict__ key) {
  const int C = src.channels();
  if ((C == 2 || C == 4 || C == 8) && ((size_t)dst & (2 * C - 1)) == 0) {
    if (ch != 0) return;
    if (C == 2)
      encode_frames<2>(src, dst, key);
    else if (C == 4)
      encode_frames<4>(src, dst, key);
    else
      encode_frames<8>(src, dst, key);
    return;
  }
  encode_scattered(src, ch, dst, key);
}
template <class Src>
__device__ __forceinline__ void encode_interleaved(const S24& fmt, const Src& src, int ch, unsigned char* __restrict__ dst,
                                                   const unsigned long long* __restrict__ key) {
  encode_flat(fmt, src, ch, dst, key);
}

}  // namespace
