// Fused quantile (pinball) loss, forward + backward.
//
// Semantics match reference resource-estimation/qrnn.py:58-67 for equal-sized
// metrics: loss = (1/(B*T*M)) * sum_{b,t,m,q} max((q-1)e, q*e), e = y - o_q.
// Forward is one grid-stride pass with wave+block reduction and a single
// atomicAdd per block; backward is pure elementwise.
//
// Templated on the output dtype: under bf16 autocast the model's (B,T,M,Q)
// predictions feed the loss DIRECTLY (math still fp32 in-register), instead
// of paying a ~280 MB f32 cast of the output tensor each step (the gradient
// is sign(e)-based quantile constants, so bf16 inputs lose nothing).
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace dr {

template <typename T, int QMAX>
__global__ void pinball_fwd_kernel(const T* __restrict__ out,      // (N, Q)
                                   const float* __restrict__ labels,  // (N,)
                                   const float* __restrict__ quantiles, int Q,
                                   int64_t N, float inv_count,
                                   float* __restrict__ loss) {
  float q[QMAX];
  for (int i = 0; i < Q; ++i) q[i] = quantiles[i];
  float acc = 0.f;
  for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N;
       n += (int64_t)gridDim.x * blockDim.x) {
    const float y = labels[n];
    const T* o = out + n * Q;
    for (int i = 0; i < Q; ++i) {
      float e = y - ldf(o + i);
      acc += fmaxf((q[i] - 1.f) * e, q[i] * e);
    }
  }
  acc = wave_sum(acc);
  __shared__ float partials[16];
  const int wave = threadIdx.x / DR_WAVE;
  const int lane = threadIdx.x % DR_WAVE;
  if (lane == 0) partials[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int wv = 0; wv < blockDim.x / DR_WAVE; ++wv) s += partials[wv];
    atomicAdd(loss, s * inv_count);
  }
}

template <typename T, int QMAX>
__global__ void pinball_bwd_kernel(const T* __restrict__ out,
                                   const float* __restrict__ labels,
                                   const float* __restrict__ quantiles, int Q,
                                   int64_t N, const float* __restrict__ grad_loss,
                                   float inv_n, T* __restrict__ dout) {
  // upstream grad read on-device (no host .item() sync -> hipGraph-capturable)
  const float gscale = grad_loss[0] * inv_n;
  float q[QMAX];
  for (int i = 0; i < Q; ++i) q[i] = quantiles[i];
  for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N;
       n += (int64_t)gridDim.x * blockDim.x) {
    const float y = labels[n];
    const T* o = out + n * Q;
    T* d = dout + n * Q;
    for (int i = 0; i < Q; ++i) {
      float e = y - ldf(o + i);
      // d/do max((q-1)e, qe): e>0 -> -q ; e<0 -> (1-q) ; e==0 -> 0
      float g = (e > 0.f) ? -q[i] : ((e < 0.f) ? (1.f - q[i]) : 0.f);
      stf(d + i, gscale * g);
    }
  }
}

// ---------------------------------------------------------------- masked
// Missing labels: a label is PRESENT iff it is finite.  Metrics then differ in
// size, so the loss is the mean over metrics (those with any present label) of
// each metric's own mean:
//   loss = (1/Mp) * sum_{m: cnt[m]>0} (sum_{present} l[.,.,m]) / cnt[m]
//   d loss / d o[b,t,m,q] = w[m] * g,  w[m] = 1/(Mp*cnt[m]),  0 where missing.
//
// The labels are an (R = B*T, M) matrix.  A block covers a tile of CW <= 256
// columns with RW = 256/CW row lanes; thread tid owns column tid % CW for its
// whole strip of rows (no modulo in the loop; consecutive threads read
// consecutive addresses).  Per-thread partial sums (fp32) and counts (int)
// meet in LDS, a tree over the row lanes folds them, and row lane 0 flushes
// once per column: one atomic per (block, metric) and accumulator into the
// zero-initialised (M,) workspaces (16 copies of them for M <= 256, see
// dr_pinball_masked_slots).  A second one-block launch turns the workspaces
// into the loss and w[m].  Missing positions are dropped by
// select, never by a 0/1 multiply: whatever the label and the outputs hold
// there (NaN, Inf) reaches neither a sum nor a gradient.

#define DR_PB_THREADS 256

__device__ __forceinline__ bool label_present(float y) {
  // finite <=> exponent field not all ones (bit test: immune to fast-math)
  return (__float_as_uint(y) & 0x7f800000u) != 0x7f800000u;
}

template <typename T, int QMAX>
__global__ void pinball_masked_fwd_kernel(const T* __restrict__ out,       // (R, M, Q)
                                          const float* __restrict__ labels,  // (R, M)
                                          const float* __restrict__ quantiles,
                                          int Q, int64_t R, int M, int CW, int RW,
                                          int S,
                                          float* __restrict__ wsum,   // (S, M)
                                          int* __restrict__ wcnt) {   // (S, M)
  __shared__ float s_sum[DR_PB_THREADS];
  __shared__ int s_cnt[DR_PB_THREADS];
  float q[QMAX];
  for (int i = 0; i < Q; ++i) q[i] = quantiles[i];
  const int tid = threadIdx.x;
  const int rl = tid / CW;                 // row lane
  const int col = blockIdx.x * CW + (tid - rl * CW);
  float acc = 0.f;
  int cnt = 0;
  if (rl < RW && col < M) {
    for (int64_t r = (int64_t)blockIdx.y * RW + rl; r < R;
         r += (int64_t)gridDim.y * RW) {
      const int64_t n = r * M + col;
      // label and outputs are loaded together (one memory round trip per
      // row, not two); what a missing position holds is dropped by select
      const float y = labels[n];
      const T* o = out + n * Q;
      float l = 0.f;
      for (int i = 0; i < Q; ++i) {
        float e = y - ldf(o + i);
        l += fmaxf((q[i] - 1.f) * e, q[i] * e);
      }
      const bool present = label_present(y);
      acc += present ? l : 0.f;
      cnt += present ? 1 : 0;
    }
  }
  s_sum[tid] = acc;
  s_cnt[tid] = cnt;
  __syncthreads();
  // fold row lanes [s, 2s) onto [0, s); RW need not be a power of two
  int half = 1;
  while (half < RW) half <<= 1;
  for (int s = half >> 1; s > 0; s >>= 1) {
    if (rl < s && rl + s < RW) {
      s_sum[tid] += s_sum[tid + s * CW];
      s_cnt[tid] += s_cnt[tid + s * CW];
    }
    __syncthreads();
  }
  if (rl == 0 && col < M && s_cnt[tid] > 0) {
    // blocks of one column tile spread over S copies of the workspace: with a
    // small M every block would otherwise add into the same few cache lines
    const int64_t slot = (int64_t)(blockIdx.y % S) * M + col;
    atomicAdd(wsum + slot, s_sum[tid]);
    atomicAdd(wcnt + slot, s_cnt[tid]);
  }
}

// one block: workspaces -> loss and the per-metric gradient weights
__global__ void pinball_masked_finalize_kernel(const float* __restrict__ wsum,
                                               const int* __restrict__ wcnt,
                                               int M, int S,
                                               float* __restrict__ loss,
                                               float* __restrict__ w) {
  __shared__ float s_per[DR_PB_THREADS / DR_WAVE];
  __shared__ int s_mp[DR_PB_THREADS / DR_WAVE];
  float per = 0.f;
  int mp = 0;
  for (int m = threadIdx.x; m < M; m += blockDim.x) {
    int c = 0;
    float sum = 0.f;
    for (int k = 0; k < S; ++k) {
      c += wcnt[(int64_t)k * M + m];
      sum += wsum[(int64_t)k * M + m];
    }
    if (c > 0) {
      per += sum / (float)c;
      ++mp;
    }
  }
  per = wave_sum(per);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mp += __shfl_xor(mp, off, DR_WAVE);
  const int wave = threadIdx.x / DR_WAVE;
  if (threadIdx.x % DR_WAVE == 0) {
    s_per[wave] = per;
    s_mp[wave] = mp;
  }
  __syncthreads();
  per = 0.f;
  mp = 0;
  for (int wv = 0; wv < DR_PB_THREADS / DR_WAVE; ++wv) {
    per += s_per[wv];
    mp += s_mp[wv];
  }
  if (threadIdx.x == 0) loss[0] = mp > 0 ? per / (float)mp : 0.f;
  for (int m = threadIdx.x; m < M; m += blockDim.x) {
    int c = 0;
    for (int k = 0; k < S; ++k) c += wcnt[(int64_t)k * M + m];
    w[m] = c > 0 ? 1.f / ((float)mp * (float)c) : 0.f;
  }
}

// same thread layout as the forward: w[col] is read once per thread
template <typename T, int QMAX>
__global__ void pinball_masked_bwd_kernel(const T* __restrict__ out,
                                          const float* __restrict__ labels,
                                          const float* __restrict__ quantiles,
                                          int Q, int64_t R, int M, int CW, int RW,
                                          const float* __restrict__ grad_loss,
                                          const float* __restrict__ w,
                                          T* __restrict__ dout) {
  const int tid = threadIdx.x;
  const int rl = tid / CW;
  const int col = blockIdx.x * CW + (tid - rl * CW);
  if (rl >= RW || col >= M) return;
  const float gscale = grad_loss[0] * w[col];
  float q[QMAX];
  for (int i = 0; i < Q; ++i) q[i] = quantiles[i];
  for (int64_t r = (int64_t)blockIdx.y * RW + rl; r < R;
       r += (int64_t)gridDim.y * RW) {
    const int64_t n = r * M + col;
    const float y = labels[n];
    const bool present = label_present(y);
    const T* o = out + n * Q;
    T* d = dout + n * Q;
    for (int i = 0; i < Q; ++i) {
      float e = y - ldf(o + i);
      float g = (e > 0.f) ? -q[i] : ((e < 0.f) ? (1.f - q[i]) : 0.f);
      stf(d + i, present ? gscale * g : 0.f);
    }
  }
}

// Launch geometry of the masked kernels: the fewest column tiles of at most
// 256 columns, evenly sized; the rest of the block goes to row lanes, so a
// small M still fills the block.  grid.y splits the rows, at least
// `rows_per_thread` rows to a thread, at most ~2048 blocks in all.
struct MaskedGeom {
  int cw, rw, block;
  dim3 grid;
};

static MaskedGeom masked_geom(int64_t R, int M, int rows_per_thread) {
  MaskedGeom g;
  const int tiles = (M + DR_PB_THREADS - 1) / DR_PB_THREADS;
  g.cw = (M + tiles - 1) / tiles;
  g.rw = DR_PB_THREADS / g.cw;
  g.block = (g.cw * g.rw + DR_WAVE - 1) / DR_WAVE * DR_WAVE;
  const int64_t strip = (int64_t)g.rw * rows_per_thread;
  const int64_t cap = std::max<int64_t>(2048 / tiles, 1);
  const int64_t ny = std::min<int64_t>(std::max<int64_t>((R + strip - 1) / strip, 1), cap);
  g.grid = dim3((unsigned)tiles, (unsigned)ny);
  return g;
}

// the unmasked kernels: grid-stride over N, at least one block
static dim3 pinball_grid(int64_t N) {
  return dim3((unsigned)std::max<int64_t>(std::min<int64_t>((N + 255) / 256, 2048), 1));
}

}  // namespace dr

// Entry contracts: kernels.h.
extern "C" {

int dr_pinball_masked_slots(int M) { return M <= DR_PB_THREADS ? 16 : 1; }

int dr_pinball_masked_fwd(const void* out, const float* labels,
                          const float* quantiles, int Q, int64_t R, int M,
                          float* wsum, int* wcnt, float* loss, float* w,
                          int is_bf16, hipStream_t stream) {
  const dr::MaskedGeom g = dr::masked_geom(R, M, 4);
  const int S = dr_pinball_masked_slots(M);
  return (int)dr::with_io_type(is_bf16, [&](auto io) {
    using T = typename decltype(io)::type;
    hipLaunchKernelGGL((dr::pinball_masked_fwd_kernel<T, 8>), g.grid,
                       dim3(g.block), 0, stream, (const T*)out, labels,
                       quantiles, Q, R, M, g.cw, g.rw, S, wsum, wcnt);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(dr::pinball_masked_finalize_kernel, dim3(1),
                       dim3(DR_PB_THREADS), 0, stream, wsum, wcnt, M, S, loss,
                       w);
    return hipGetLastError();
  });
}

int dr_pinball_masked_bwd(const void* out, const float* labels,
                          const float* quantiles, int Q, int64_t R, int M,
                          const float* grad_loss, const float* w, void* dout,
                          int is_bf16, hipStream_t stream) {
  const dr::MaskedGeom g = dr::masked_geom(R, M, 1);
  return (int)dr::with_io_type(is_bf16, [&](auto io) {
    using T = typename decltype(io)::type;
    hipLaunchKernelGGL((dr::pinball_masked_bwd_kernel<T, 8>), g.grid,
                       dim3(g.block), 0, stream, (const T*)out, labels,
                       quantiles, Q, R, M, g.cw, g.rw, grad_loss, w, (T*)dout);
    return hipGetLastError();
  });
}

int dr_pinball_fwd(const void* out, const float* labels, const float* quantiles,
                   int Q, int64_t N, float inv_count, float* loss, int is_bf16,
                   hipStream_t stream) {
  return (int)dr::with_io_type(is_bf16, [&](auto io) {
    using T = typename decltype(io)::type;
    hipLaunchKernelGGL((dr::pinball_fwd_kernel<T, 8>), dr::pinball_grid(N),
                       dim3(256), 0, stream, (const T*)out, labels, quantiles, Q,
                       N, inv_count, loss);
    return hipGetLastError();
  });
}

int dr_pinball_bwd(const void* out, const float* labels, const float* quantiles,
                   int Q, int64_t N, const float* grad_loss, float inv_n,
                   void* dout, int is_bf16, hipStream_t stream) {
  return (int)dr::with_io_type(is_bf16, [&](auto io) {
    using T = typename decltype(io)::type;
    hipLaunchKernelGGL((dr::pinball_bwd_kernel<T, 8>), dr::pinball_grid(N),
                       dim3(256), 0, stream, (const T*)out, labels, quantiles, Q,
                       N, grad_loss, inv_n, (T*)dout);
    return hipGetLastError();
  });
}

}  // extern "C"

