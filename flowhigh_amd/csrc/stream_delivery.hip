// Streaming delivery (FlowHighSR.stream(delivery=), FlowHighSR.delivery_stream; flowhigh_amd/stream_delivery.py is the schedule
// and the definition): the delivery of a stream block by block, with the bits of the one-shot delivery of the whole stream.
//   fh_stream_resample_f32   the polyphase resampler (frontend.hip: resample_poly_kernel's loop and order) on absolute indices
//   fh_stream_limit_f32      the oversampled envelope and the look-ahead limiter of mono streams in one launch
//                            (truepeak.hip: tp_envelope_kernel + limit_kernel, their arithmetic and order)
//   fh_stream_pcm_i16_f32    the PCM encoder (pcm_common.h: pcm.hip's bodies) with the dither at the sample's absolute index
//   fh_stream_limit_linked_f32   the limiter of streams of 1 .. 8 channels: one envelope and one gain for a stream's channels
//   fh_stream_pcm_i16_rows_f32   the encoder of such streams: channel c's dither, planar rows or interleaved sample frames
//   fh_stream_pcm_s24_rows_f32   the same kernel in 24 bits (packed in 3 bytes or in an int32), for mono streams too: a group of
//                                one job
// One fh_stream_job per row and launch.  A job's source is TWO spans, the carry the stream kept and the fresh block, read as
// one run of samples whose first has the absolute index `base`; nothing is concatenated.  The last block column of a launch
// copies the last n_keep source samples into the stream's other carry buffer (the two ping-pong, so the copy never writes
// what the launch reads).
//
// The job table lives on the device: a kernel returns at once on a job with a negative count or a null pointer it would use,
// reads the source only through sd_src::at (0 outside the two spans) and writes only dst[0 .. n_out) and carry_out[0 .. n_keep).
//
// Groups: a stream of C channels is a group of C consecutive jobs, one per channel row, with equal base, first and counts.  The
// limiter and the encoder are ONE kernel each, instantiated with a group locator (the encoder with a sample format of
// pcm_common.h as well, whose bodies do all of its arithmetic and stores): OneJob for the mono entries (job g alone is
// group g: C = 1, no table is read), GroupTable for the other two (a device table `groups` of int32 [n_groups + 1] gives every
// stream's first job; a group whose size is not 1 .. 8, whose jobs differ in a counter or one of whose jobs fails job_ok is left
// unwritten).  So a mono stream has the bits of a stream of one channel.  The resampler runs a row per job as it is.
//
// Limiter: a workgroup owns TILE outputs of one group from `first` on.  Channel by channel, the samples of tile +- (2 H + HALO) go
// to the one xs buffer in LDS (0 before the stream's sample 0, and past its last one when it has ended) and the channel's peaks
// are folded with fmaxf in tp_envelope_kernel's order (best = 0, then channel 0, 1, ...) into one m per sample of tile +- 2 H; the
// last channel's pass turns m into r (1 outside the stream).  Then the sliding minimum and the float64 Hann sum run once per tile
// (gain_tile, which limit_kernel calls too), and every channel's x takes the one g: the last channel's from xs, which still holds
// it, the others' read again from their source.  The envelope work is (TILE + 4 H) / TILE of that of the two launches on a clip:
// the price of one launch and no m round trip.
#include "fh_common.h"
#include "pcm_common.h"
#include "truepeak_common.h"

namespace {

using namespace tp;                             // (truepeak_common.h: THREADS, the limiter's TILE outputs per workgroup, ...)
constexpr int MAX_CH = 8;                       // channels of a stream
static_assert(THREADS == PCM_THREADS, "the encoder bodies count their runs in blocks of PCM_THREADS");

struct sd_src {                                 // the two spans as one run of samples
  const float* carry;
  const float* fresh;
  long long base;
  int n_carry, n_fresh;
  __device__ long long end() const { return base + n_carry + n_fresh; }
  __device__ float at(long long a) const {      // sample a of the stream; 0 outside the spans
    const long long s = a - base;
    if (s < 0) return 0.f;
    if (s < n_carry) return carry[s];
    const long long f = s - n_carry;
    return f < n_fresh ? fresh[f] : 0.f;
  }
};

__device__ __forceinline__ bool job_ok(const fh_stream_job& J) {
  return J.n_carry >= 0 && J.n_fresh >= 0 && J.n_out >= 0 && J.n_keep >= 0 && J.base >= 0 && J.first >= 0 &&
         (J.n_carry == 0 || J.carry) && (J.n_fresh == 0 || J.fresh) && (J.n_out == 0 || J.dst) && (J.n_keep == 0 || J.carry_out) &&
         (long long)J.n_keep <= (long long)J.n_carry + J.n_fresh;
}

__device__ __forceinline__ sd_src source(const fh_stream_job& J) {
  return {(const float*)J.carry, (const float*)J.fresh, J.base, J.n_carry, J.n_fresh};
}

// carry_out[s] = the source's sample end - n_keep + s, by one workgroup
__device__ __forceinline__ void keep_tail(const fh_stream_job& J, const sd_src& S) {
  float* __restrict__ out = (float*)J.carry_out;
  const long long from = S.end() - J.n_keep;
  for (int s = threadIdx.x; s < J.n_keep; s += THREADS) out[s] = S.at(from + s);
}

// out[i] = sum_j x[j] * h[(i + pre) * down - j * up] for i = first + o: resample_poly_kernel's loop on 64-bit indices, its j_hi
// clamped to the last sample that is there (the stream's last one when it has ended; the schedule asks for no other output)
__global__ __launch_bounds__(THREADS) void stream_resample_kernel(const fh_stream_job* __restrict__ jobs, const float* __restrict__ h,
                                                                  int up, int down, int n_taps, int pre) {
  const fh_stream_job J = jobs[blockIdx.y];
  if (!job_ok(J)) return;
  const sd_src S = source(J);
  if (blockIdx.x == gridDim.x - 1) {
    keep_tail(J, S);
    return;
  }
  const long long o = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (o >= J.n_out) return;
  const long long pos = (J.first + o + pre) * down;
  long long j_hi = pos / up;
  if (j_hi > S.end() - 1) j_hi = S.end() - 1;
  float acc = 0.f;
  for (long long j = j_hi; j >= 0; --j) {
    const long long k = pos - j * up;
    if (k >= n_taps) break;
    acc = fmaf(S.at(j), h[k], acc);
  }
  ((float*)J.dst)[o] = acc;
}

// The jobs [j0, j0 + n) of one stream: one per channel row
struct sd_group {
  int j0, n;
};

// The group locators: group(g, G) gives group g, checked (false: it is left unwritten), group_of(j) the group that may hold job j,
// and `interleaved` says whether the encoder writes sample frames (a constant 0 where none can occur).
struct OneJob {                                 // job g alone is group g
  const fh_stream_job* jobs;
  static constexpr int interleaved = 0;
  __device__ bool group(int g, sd_group& G) const {
    G = {g, 1};
    const fh_stream_job J = jobs[g];            // (the whole record in one read, not field by field as job_ok asks)
    return job_ok(J);
  }
  __device__ int group_of(int job) const { return job; }
};
struct GroupTable {                             // groups[g] .. groups[g + 1] of the device table
  const fh_stream_job* jobs;
  int n_jobs;
  const int32_t* groups;
  int n_groups, interleaved;
  // 1 .. 8 jobs inside the job table, each job_ok, all with the counters of the first (the tables live on the device)
  __device__ bool group(int g, sd_group& G) const {
    const int j0 = groups[g], j1 = groups[g + 1];
    if (j0 < 0 || j1 > n_jobs || j1 <= j0 || j1 - j0 > MAX_CH) return false;
    const fh_stream_job A = jobs[j0];
    for (int j = j0; j < j1; ++j) {
      const fh_stream_job J = jobs[j];
      if (!job_ok(J) || J.base != A.base || J.first != A.first || J.n_carry != A.n_carry || J.n_fresh != A.n_fresh ||
          J.n_out != A.n_out || J.n_keep != A.n_keep)
        return false;
    }
    G = {j0, j1 - j0};
    return true;
  }
  __device__ int group_of(int job) const {      // the last group that starts at or below the job, by bisection
    int g = 0, hi = n_groups;
    while (hi - g > 1) {
      const int mid = (g + hi) >> 1;
      if (groups[mid] <= job)
        g = mid;
      else
        hi = mid;
    }
    return g;
  }
};

// A workgroup owns one tile of one group.  a[0][j] collects m over the channels (the thread that owns j is the same in every
// pass) and becomes r in the last channel's pass.
template <class Groups>
__global__ __launch_bounds__(THREADS) void stream_limit_kernel(Groups groups, const float* __restrict__ taps, const double* __restrict__ w,
                                                               int H, float c32) {
  __shared__ float xs[LIM_N + 2 * HALO];
  __shared__ float hs[4][PHASE_TAPS];
  __shared__ float a[2][LIM_N];
  __shared__ double ws[2 * MAX_H + 1];
  sd_group G;
  if (!groups.group(blockIdx.y, G)) return;
  const fh_stream_job* __restrict__ jobs = groups.jobs + G.j0;
  if (blockIdx.x == gridDim.x - 1) {
    for (int c = 0; c < G.n; ++c) {
      const fh_stream_job J = jobs[c];
      keep_tail(J, source(J));
    }
    return;
  }
  const fh_stream_job J0 = jobs[0];                                  // (the counters are the group's)
  const long long rel0 = (long long)blockIdx.x * TILE;               // the tile's first output in every dst
  if (rel0 >= J0.n_out) return;
  const long long tile0 = J0.first + rel0, end = source(J0).end();
  const int t = threadIdx.x, N = TILE + 4 * H;
  load_taps(taps, hs);
  for (int j = t; j < 2 * H + 1; j += THREADS) ws[j] = w[j];
  for (int c = 0; c < G.n; ++c) {                                    // a[0][j] = m[tile0 - 2 H + j]: best = 0, then channel by channel
    const sd_src S = source(jobs[c]);
    for (int j = t; j < N + 2 * HALO; j += THREADS) xs[j] = S.at(tile0 - 2 * H - HALO + j);      // (0 before sample 0 and past `end`)
    __syncthreads();
    for (int j = t; j < N; j += THREADS) {
      const long long n = tile0 - 2 * H + j;
      const bool last = c == G.n - 1;
      float mv = c ? a[0][j] : 0.f, r = 1.f;                           // r[tile0 - 2 H + j]; 1 outside the stream
      if (n >= 0 && n < end) {
        mv = fmaxf(mv, peak_at(xs, hs, j));
        if (last && mv > c32) r = __fdiv_rn(c32, mv);                  // (a branch: few samples are over the ceiling)
      }
      a[0][j] = last ? r : mv;
    }
    __syncthreads();                                                 // (xs is staged again, or a[0] is read)
  }
  double acc[PER];
  gain_tile(a, ws, H, acc);
  for (int c = 0; c < G.n; ++c) {                                    // (xs holds the last channel, the others are read again)
    const fh_stream_job J = jobs[c];
    const sd_src S = source(J);
    float* __restrict__ dst = (float*)J.dst + rel0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = t + k * THREADS;
      if (rel0 + i < J.n_out) dst[i] = limit_sample(c == G.n - 1 ? xs[i + 2 * H + HALO] : S.at(tile0 + i), (float)acc[k], c32);
    }
  }
}

// The jobs of a checked group as the encoder bodies see them: the source of pcm_common.h over the two spans of every job.  The
// counters are the group's (its jobs have equal ones); output o of a job is the stream's sample first + o.
struct stream_rows {
  const fh_stream_job* jobs;                    // channel c is jobs[c]
  long long first;
  int n, n_out;
  __device__ int channels() const { return n; }
  __device__ int len() const { return n_out; }
  __device__ long long origin() const { return first; }
  __device__ float at(int ch, long long o) const { return source(jobs[ch]).at(first + o); }
  __device__ void load_run(int ch, long long o0, float (&x)[RUN]) const {
    const fh_stream_job J = jobs[ch];
    const sd_src S = source(J);
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
      const long long o = o0 + k;
      x[k] = (o >= 0 && o < n_out) ? S.at(first + o) : 0.f;
    }
  }
};

// The encoder: pcm.hip's kernel on a stream's blocks, with the dither at the sample's absolute index.  Grid (blocks of 256 runs,
// jobs): job j is channel j - G.j0 of the group that holds it (a job no group holds, or whose group is refused, is left
// unwritten) and takes the group's key.  Planar: every job writes its own dst, none if a dst of the group is misaligned for the
// format.  Interleaved: the group's first dst is the frame buffer [n_out, C].  The samples, the dither and the stores are the
// bodies of pcm_common.h.
template <class Groups, class Fmt>
__global__ __launch_bounds__(THREADS) void stream_pcm_kernel(Groups groups, Fmt fmt, const unsigned long long* __restrict__ keys) {
  const int job = blockIdx.y, g = groups.group_of(job);
  sd_group G;
  if (!groups.group(g, G) || job < G.j0 || job >= G.j0 + G.n) return;
  const fh_stream_job* __restrict__ jobs = groups.jobs + G.j0;
  const int ch = job - G.j0;
  for (int c = 0; c < (groups.interleaved ? 1 : G.n); ++c)
    if (!fmt.ok(jobs[c].dst)) return;
  const stream_rows src{jobs, jobs[0].first, G.n, jobs[0].n_out};
  const unsigned long long* __restrict__ key = keys ? keys + 2 * g : nullptr;
  if (groups.interleaved)
    encode_interleaved(fmt, src, ch, (unsigned char*)jobs[0].dst, key);
  else
    encode_row(fmt, src, ch, (unsigned char*)jobs[ch].dst, key);
}

}  // namespace

extern "C" int fh_sizeof_stream_job(void) { return (int)sizeof(fh_stream_job); }

#define FH_CHECK_STREAM_JOBS(name)                                                                   \
  FH_CHECK_ARG(jobs, name ": null job table");                                                       \
  FH_CHECK_ARG(n_jobs > 0 && n_jobs < 65536, name ": %d jobs (1 .. 65535)", n_jobs);                 \
  FH_CHECK_ARG(max_out >= 0, name ": max_out %d must not be negative", max_out)

extern "C" int fh_stream_resample_f32(const fh_stream_job* jobs, int n_jobs, int max_out, const float* taps, int up, int down,
                                      int n_taps, int pre, void* stream) {
  FH_CHECK_STREAM_JOBS("fh_stream_resample_f32");
  FH_CHECK_ARG(taps, "fh_stream_resample_f32: null taps");
  FH_CHECK_ARG(up > 0 && down > 0 && n_taps > 0 && pre >= 0, "fh_stream_resample_f32: up %d, down %d, n_taps %d must be positive, "
               "pre %d not negative", up, down, n_taps, pre);
  hipLaunchKernelGGL(stream_resample_kernel, dim3(fh_cdiv(max_out, THREADS) + 1, n_jobs), dim3(THREADS), 0, (hipStream_t)stream, jobs,
                     taps, up, down, n_taps, pre);
  FH_CHECK_LAUNCH("fh_stream_resample_f32");
  return FH_OK;
}

#define FH_CHECK_STREAM_LIMIT(name)                                                                                        \
  FH_CHECK_ARG(taps4 && w, name ": null pointer (taps4 %p, w %p)", (const void*)taps4, (const void*)w);                    \
  FH_CHECK_ARG(H >= 1 && H <= MAX_H, name ": H %d (1 .. %d)", H, MAX_H);                                                   \
  FH_CHECK_ARG(ceiling > 0.f && ceiling <= 1.f, name ": ceiling %g (0 < c <= 1)", (double)ceiling);                       \
  FH_CHECK_ARG((((size_t)taps4) & 3) == 0 && (((size_t)w) & 7) == 0, name ": taps4 must be 4-byte, w 8-byte aligned")

#define FH_CHECK_STREAM_GROUPS(name)                                                                                       \
  FH_CHECK_ARG(groups, name ": null group table");                                                                        \
  FH_CHECK_ARG(n_groups > 0 && n_groups < 65536, name ": %d groups (1 .. 65535)", n_groups);                              \
  FH_CHECK_ARG((((size_t)groups) & 3) == 0, name ": groups must be 4-byte aligned")

extern "C" int fh_stream_limit_f32(const fh_stream_job* jobs, int n_jobs, int max_out, const float* taps4, const double* w, int H,
                                   float ceiling, void* stream) {
  FH_CHECK_STREAM_JOBS("fh_stream_limit_f32");
  FH_CHECK_STREAM_LIMIT("fh_stream_limit_f32");
  hipLaunchKernelGGL(stream_limit_kernel<OneJob>, dim3(fh_cdiv(max_out, TILE) + 1, n_jobs), dim3(THREADS), 0, (hipStream_t)stream,
                     OneJob{jobs}, taps4, w, H, ceiling);
  FH_CHECK_LAUNCH("fh_stream_limit_f32");
  return FH_OK;
}

extern "C" int fh_stream_pcm_i16_f32(const fh_stream_job* jobs, int n_jobs, int max_out, const uint64_t* keys, void* stream) {
  FH_CHECK_STREAM_JOBS("fh_stream_pcm_i16_f32");
  hipLaunchKernelGGL((stream_pcm_kernel<OneJob, I16>), dim3(pcm_blocks(max_out), n_jobs), dim3(THREADS), 0, (hipStream_t)stream,
                     OneJob{jobs}, I16{}, (const unsigned long long*)keys);
  FH_CHECK_LAUNCH("fh_stream_pcm_i16_f32");
  return FH_OK;
}

extern "C" int fh_stream_limit_linked_f32(const fh_stream_job* jobs, int n_jobs, const int32_t* groups, int n_groups, int max_out,
                                          const float* taps4, const double* w, int H, float ceiling, void* stream) {
  FH_CHECK_STREAM_JOBS("fh_stream_limit_linked_f32");
  FH_CHECK_STREAM_GROUPS("fh_stream_limit_linked_f32");
  FH_CHECK_STREAM_LIMIT("fh_stream_limit_linked_f32");
  hipLaunchKernelGGL(stream_limit_kernel<GroupTable>, dim3(fh_cdiv(max_out, TILE) + 1, n_groups), dim3(THREADS), 0, (hipStream_t)stream,
                     GroupTable{jobs, n_jobs, groups, n_groups, 0}, taps4, w, H, ceiling);
  FH_CHECK_LAUNCH("fh_stream_limit_linked_f32");
  return FH_OK;
}

extern "C" int fh_stream_pcm_i16_rows_f32(const fh_stream_job* jobs, int n_jobs, const int32_t* groups, int n_groups, int max_out,
                                          const uint64_t* keys, int interleaved, void* stream) {
  FH_CHECK_STREAM_JOBS("fh_stream_pcm_i16_rows_f32");
  FH_CHECK_STREAM_GROUPS("fh_stream_pcm_i16_rows_f32");
  hipLaunchKernelGGL((stream_pcm_kernel<GroupTable, I16>), dim3(pcm_blocks(max_out), n_jobs), dim3(THREADS), 0, (hipStream_t)stream,
                     GroupTable{jobs, n_jobs, groups, n_groups, interleaved ? 1 : 0}, I16{}, (const unsigned long long*)keys);
  FH_CHECK_LAUNCH("fh_stream_pcm_i16_rows_f32");
  return FH_OK;
}

extern "C" int fh_stream_pcm_s24_rows_f32(const fh_stream_job* jobs, int n_jobs, const int32_t* groups, int n_groups, int max_out,
                                          const uint64_t* keys, int interleaved, int container, void* stream) {
  FH_CHECK_STREAM_JOBS("fh_stream_pcm_s24_rows_f32");
  FH_CHECK_STREAM_GROUPS("fh_stream_pcm_s24_rows_f32");
  FH_CHECK_PCM_CONTAINER("fh_stream_pcm_s24_rows_f32");
  hipLaunchKernelGGL((stream_pcm_kernel<GroupTable, S24>), dim3(pcm_blocks(max_out), n_jobs), dim3(THREADS), 0, (hipStream_t)stream,
                     GroupTable{jobs, n_jobs, groups, n_groups, interleaved ? 1 : 0}, S24{container}, (const unsigned long long*)keys);
  FH_CHECK_LAUNCH("fh_stream_pcm_s24_rows_f32");
  return FH_OK;
}
