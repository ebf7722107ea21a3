// Sanity check on the device: normalized quantile output + measured
// utilization -> exceedance scores, debounced flags and per-(window, metric)
// summaries, in one memory-bound pass.
//
// Per (n, t, m) the band is what Predictor.predict_tensor serves, step for
// step: add the ridge base, sort the triple, widen by the conformal score
// (clamped at the median), inverse-scale, expm1 (log1p targets), clamp at
// 1e-6.  The score is AnomalyScorer.score's: max((y - q2) / max(q2 - q0,
// 1e-9), 0); a position is `over` when its score exceeds the threshold, and
// flagged when it lies in a run of at least min_run consecutive overs.
//
// Every operation is a single correctly rounded f32 op in the order of the
// torch composition (no fma contraction, IEEE divide, libm expm1f), so the
// kernel's bands and scores track the f32 torch route to the last bits.
//
// Mapping: one thread per (n, m), m fastest across lanes, looping over t.  At
// each step a wave reads contiguous runs of out (12 B per lane in f32),
// measured and base.  The run counter lives in a register; when a run first
// reaches min_run the thread back-fills its own min_run - 1 earlier flags
// (its own addresses: program order suffices; t - (min_run - 1) >= 0 because
// a run of min_run ending at t started at or after 0).  The loads of
// DR_SANITY_AHEAD steps are issued together, one group ahead of their use.
//
// Gaps and padding are removed by select: a non-finite measured value is "not
// observed" (score NaN, not over, ends the run, in no summary but the count);
// positions t >= L are never loaded (score NaN, flag 0, bands NaN, in no
// summary; a run ends at L).  Nothing stored there can reach a valid output.
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace dr {

#define DR_SANITY_THREADS 64
#define DR_SANITY_AHEAD 4

__device__ __forceinline__ bool sanity_observed(float y) {
  // finite <=> exponent field not all ones (bit test: immune to fast-math)
  return (__float_as_uint(y) & 0x7f800000u) != 0x7f800000u;
}

__device__ __forceinline__ void ld3(const float* p, float v[3]) {
  v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
}
__device__ __forceinline__ void ld3(const uint16_t* p, float v[3]) {
  v[0] = bf2f(p[0]); v[1] = bf2f(p[1]); v[2] = bf2f(p[2]);
}

// the loads of DR_SANITY_AHEAD consecutive steps of one (n, m)
struct SanityGroup {
  float o[DR_SANITY_AHEAD][3];
  float y[DR_SANITY_AHEAD];
  float b[DR_SANITY_AHEAD];
};

template <typename T>
__device__ __forceinline__ void sanity_load(SanityGroup& g, const T* out,
                                            const float* measured,
                                            const float* base, int64_t e,
                                            int M) {
#pragma unroll
  for (int k = 0; k < DR_SANITY_AHEAD; ++k) {
    const int64_t ek = e + (int64_t)k * M;
    ld3(out + ek * 3, g.o[k]);
    g.y[k] = measured[ek];
    g.b[k] = base != nullptr ? base[ek] : 0.f;
  }
}

// what one thread carries along t
struct SanityState {
  int run = 0, n_flagged = 0, first_flag = -1, n_observed = 0;
  float max_score = 0.f;
};

struct SanityParams {
  float scale, min, conf, threshold;
  int log1p, min_run, M;
  float* scores;
  uint8_t* flags;
  float* bands;
};

// one valid step: e is the (n, t, m) element index
__device__ __forceinline__ void sanity_step(const SanityParams& p, SanityState& s,
                                            int t, int64_t e, const float o[3],
                                            float y, float b) {
  // one rounding per torch op: a multiply and the add after it stay two
  // instructions (hipcc contracts them into an fma by default), and the
  // divide is the correctly rounded one
#pragma clang fp contract(off)
  const float a0 = o[0] + b, a1 = o[1] + b, a2 = o[2] + b;
  // sort the triple
  const float lo = fminf(a0, a1), hi = fmaxf(a0, a1);
  const float mid = fminf(hi, a2);
  float q2 = fmaxf(hi, a2);
  float q0 = fminf(lo, mid);
  float q1 = fmaxf(lo, mid);
  // conformal widening, clamped at the median (conf == 0: unchanged)
  q0 = fminf(q0 - p.conf, q1);
  q2 = fmaxf(q2 + p.conf, q1);
  q0 = q0 * p.scale + p.min;
  q1 = q1 * p.scale + p.min;
  q2 = q2 * p.scale + p.min;
  if (p.log1p) {
    q0 = expm1f(q0);
    q1 = expm1f(q1);
    q2 = expm1f(q2);
  }
  q0 = fmaxf(q0, 1e-6f);
  q1 = fmaxf(q1, 1e-6f);
  q2 = fmaxf(q2, 1e-6f);
  if (p.bands != nullptr) {
    float* bp = p.bands + e * 3;
    bp[0] = q0; bp[1] = q1; bp[2] = q2;
  }
  const float band = fmaxf(q2 - q0, 1e-9f);
  const float score = fmaxf((y - q2) / band, 0.f);
  const bool obs = sanity_observed(y);
  const bool over = obs && score > p.threshold;
  p.scores[e] = obs ? score : __uint_as_float(0x7fc00000u);
  s.n_observed += obs ? 1 : 0;
  s.max_score = obs ? fmaxf(s.max_score, score) : s.max_score;
  s.run = over ? s.run + 1 : 0;
  const bool flagged = s.run >= p.min_run;
  p.flags[e] = flagged ? 1 : 0;
  if (flagged) {
    if (s.run == p.min_run) {
      // the run has just become long enough: flag its earlier positions.
      // run <= t + 1, so t - (min_run - 1) >= 0.
      for (int j = 1; j < p.min_run; ++j) p.flags[e - (int64_t)j * p.M] = 1;
      s.n_flagged += p.min_run - 1;
      if (s.first_flag < 0) s.first_flag = t - (p.min_run - 1);
    }
    s.n_flagged += 1;
  }
}

template <typename T>
__global__ void __launch_bounds__(DR_SANITY_THREADS)
sanity_kernel(const T* __restrict__ out,            // (N, TT, M, 3)
              const float* __restrict__ measured,   // (N, TT, M)
              const float* __restrict__ base,       // (N, TT, M) or null
              const float* __restrict__ y_min,      // (M,)
              const float* __restrict__ y_scale,    // (M,)
              const float* __restrict__ conformal,  // (M,) or null
              const int* __restrict__ lengths,      // (N,) or null
              int64_t NM, int TT, int M, int log1p, float threshold,
              int min_run,
              float* __restrict__ scores,           // (N, TT, M)
              uint8_t* __restrict__ flags,          // (N, TT, M)
              float* __restrict__ max_score,        // (N, M)
              int* __restrict__ n_flagged, int* __restrict__ first_flag,
              int* __restrict__ n_observed,
              float* __restrict__ bands) {          // (N, TT, M, 3) or null
  const int64_t idx = (int64_t)blockIdx.x * DR_SANITY_THREADS + threadIdx.x;
  if (idx >= NM) return;
  const int64_t n = idx / M;
  const int m = (int)(idx - n * M);
  int L = TT;
  if (lengths != nullptr) L = min(max(lengths[n], 1), TT);

  SanityParams p;
  p.scale = y_scale[m];
  p.min = y_min[m];
  p.conf = conformal != nullptr ? conformal[m] : 0.f;
  p.threshold = threshold;
  p.log1p = log1p;
  p.min_run = min_run;
  p.M = M;
  p.scores = scores;
  p.flags = flags;
  p.bands = bands;
  SanityState s;

  const int64_t e0 = n * TT * M + m;     // element (n, 0, m); one step is +M
  const int groups = L / DR_SANITY_AHEAD;
  SanityGroup cur, nxt;
  if (groups > 0) sanity_load(cur, out, measured, base, e0, M);
  for (int g = 0; g < groups; ++g) {
    // next group's loads go out before this group is used; the last
    // iteration re-reads its own group (in bounds, no branch round the loads)
    const int gn = min(g + 1, groups - 1);
    sanity_load(nxt, out, measured, base,
                e0 + (int64_t)gn * DR_SANITY_AHEAD * M, M);
    const int t0 = g * DR_SANITY_AHEAD;
#pragma unroll
    for (int k = 0; k < DR_SANITY_AHEAD; ++k)
      sanity_step(p, s, t0 + k, e0 + (int64_t)(t0 + k) * M, cur.o[k], cur.y[k],
                  cur.b[k]);
    cur = nxt;
  }
  int t = groups * DR_SANITY_AHEAD;
  for (; t < L; ++t) {
    const int64_t e = e0 + (int64_t)t * M;
    float o[3];
    ld3(out + e * 3, o);
    sanity_step(p, s, t, e, o, measured[e], base != nullptr ? base[e] : 0.f);
  }
  // padding: never loaded
  const float nan = __uint_as_float(0x7fc00000u);
  for (; t < TT; ++t) {
    const int64_t e = e0 + (int64_t)t * M;
    scores[e] = nan;
    flags[e] = 0;
    if (bands != nullptr) {
      float* bp = bands + e * 3;
      bp[0] = nan; bp[1] = nan; bp[2] = nan;
    }
  }
  max_score[idx] = s.max_score;
  n_flagged[idx] = s.n_flagged;
  first_flag[idx] = s.first_flag;
  n_observed[idx] = s.n_observed;
}

}  // namespace dr

// Entry contract: kernels.h.
extern "C" {

int dr_sanity_scores(const void* out, const float* measured, const float* base,
                     const float* y_min, const float* y_scale,
                     const float* conformal, const int* lengths, int64_t N,
                     int TT, int M, int log1p, float threshold, int min_run,
                     float* scores, uint8_t* flags, float* max_score,
                     int* n_flagged, int* first_flag, int* n_observed,
                     float* bands, int is_bf16, hipStream_t stream) {
  const int64_t NM = N * M;
  const dim3 grid((unsigned)((NM + DR_SANITY_THREADS - 1) / DR_SANITY_THREADS));
  const dim3 block(DR_SANITY_THREADS);
  return (int)dr::with_io_type(is_bf16, [&](auto io) {
    using T = typename decltype(io)::type;
    hipLaunchKernelGGL(dr::sanity_kernel<T>, grid, block, 0, stream,
                       (const T*)out, measured, base, y_min, y_scale, conformal,
                       lengths, NM, TT, M, log1p, threshold, min_run, scores,
                       flags, max_score, n_flagged, first_flag, n_observed,
                       bands);
    return hipGetLastError();
  });
}

}  // extern "C"
