// Fused dropout + residual-add + LayerNorm for gfx950.
//
//   r_out  = residual + (keep ? branch / (1 - p) : 0)   fp32 math, IO dtype
//   normed = LayerNorm(r_out) * w + b                    stats over the
//                                                        ROUNDED r_out
//
// One wave per row in a grid-stride row loop, a vec4 path (lane owns 4
// contiguous columns, w/b in registers across the row loop) for D % 4 == 0 &&
// D <= 256 and a strided path for every other D.  The dropout mask is never
// stored: it is Philox4x32-10 keyed on the ELEMENT index, so forward and
// backward (and a CPU oracle) generate the same bits whatever the launch
// geometry.  (key, stream) is read from device memory so a captured graph
// sees fresh values on every replay.
//
// HAS_ADD off:  plain LayerNorm of `residual` (no branch, no r_out store, no
//               d_r_out in backward); only with HAS_MASK off and HAS_NORM on.
// HAS_MASK off: p == 0 or eval, no RNG work and no seed tensor.
// HAS_NORM off: plain dropout_add (no stats, no w/b).
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace dr {

// ---- Philox4x32-10 (Salmon et al., SC'11) ----
struct PhiloxKey {
  uint32_t k0, k1;   // key
  uint32_t c2, c3;   // stream = high counter words
};

__device__ __forceinline__ PhiloxKey philox_key(const int64_t* __restrict__ seed) {
  const uint64_t key = (uint64_t)seed[0];
  const uint64_t strm = (uint64_t)seed[1];
  PhiloxKey k;
  k.k0 = (uint32_t)key;
  k.k1 = (uint32_t)(key >> 32);
  k.c2 = (uint32_t)strm;
  k.c3 = (uint32_t)(strm >> 32);
  return k;
}

// counter = (lo32(g), hi32(g), lo32(stream), hi32(stream)), g = element >> 2
__device__ __forceinline__ void philox4(uint64_t g, const PhiloxKey& pk,
                                        uint32_t out[4]) {
  uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32), c2 = pk.c2, c3 = pk.c3;
  uint32_t k0 = pk.k0, k1 = pk.k1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// keep bit of one element (strided path): output word e & 3 of group e >> 2
__device__ __forceinline__ bool philox_keep1(uint64_t e, const PhiloxKey& pk,
                                             uint32_t thr) {
  uint32_t o[4];
  philox4(e >> 2, pk, o);
  const uint32_t word = (e & 2) ? ((e & 1) ? o[3] : o[2]) : ((e & 1) ? o[1] : o[0]);
  return word >= thr;
}

// value as it reads back after a store in the IO dtype
template <typename T> __device__ __forceinline__ float round_io(float v);
template <> __device__ __forceinline__ float round_io<float>(float v) { return v; }
template <> __device__ __forceinline__ float round_io<uint16_t>(float v) { return bf2f(f2bf(v)); }

// ------------------------------------------------------------------ forward
template <typename T, bool HAS_ADD, bool HAS_MASK, bool HAS_NORM>
__global__ void __launch_bounds__(256)
dal_fwd_vec4(const T* __restrict__ branch, const T* __restrict__ residual,
             const float* __restrict__ w, const float* __restrict__ b,
             const int64_t* __restrict__ seed, uint32_t thr, float scale,
             T* __restrict__ r_out, T* __restrict__ normed,
             float* __restrict__ mean_out, float* __restrict__ rstd_out,
             int64_t n_rows, int D, float eps) {
  const int wave = threadIdx.x / DR_WAVE;
  const int lane = threadIdx.x % DR_WAVE;
  const int waves_per_block = blockDim.x / DR_WAVE;
  const int64_t row0 = (int64_t)blockIdx.x * waves_per_block + wave;
  const int64_t stride_rows = (int64_t)gridDim.x * waves_per_block;
  const int j0 = lane * 4;
  const bool active = j0 < D;
  const float invD = 1.f / D;
  float wr[4] = {0.f, 0.f, 0.f, 0.f}, br[4] = {0.f, 0.f, 0.f, 0.f};
  if (HAS_NORM && active) { ld4(w + j0, wr); ld4(b + j0, br); }
  PhiloxKey pk = {0u, 0u, 0u, 0u};
  if (HAS_MASK) pk = philox_key(seed);

  for (int64_t row = row0; row < n_rows; row += stride_rows) {
    const int64_t off = row * D + j0;   // D % 4 == 0: one Philox group
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    float a[4];
    if (HAS_ADD && active) ld4(branch + off, a);
    if (active) ld4(residual + off, v);
    if (HAS_ADD && active) {
      if (HAS_MASK) {
        uint32_t o[4];
        philox4((uint64_t)off >> 2, pk, o);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] += (o[i] >= thr) ? a[i] * scale : 0.f;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] += a[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = round_io<T>(v[i]);
      st4(r_out + off, v);
    }
    if (HAS_NORM) {
      float mu = wave_sum(v[0] + v[1] + v[2] + v[3]) * invD;
      float var = 0.f;
      if (active) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { float d = v[i] - mu; var += d * d; }
      }
      const float rstd = rsqrtf(wave_sum(var) * invD + eps);
      if (lane == 0) {
        mean_out[row] = mu;
        rstd_out[row] = rstd;
      }
      if (active) {
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (v[i] - mu) * rstd * wr[i] + br[i];
        st4(normed + off, o);
      }
    }
  }
}

// Strided path for D <= 1024: lane owns columns lane, lane + 64, ...;
// MAX_PER_LANE * 64 >= D.  The column loop is fully unrolled with a
// wave-uniform exit so the per-lane values stay in registers.
template <typename T, int MAX_PER_LANE, bool HAS_ADD, bool HAS_MASK, bool HAS_NORM>
__global__ void __launch_bounds__(256)
dal_fwd_kernel(const T* __restrict__ branch, const T* __restrict__ residual,
               const float* __restrict__ w, const float* __restrict__ b,
               const int64_t* __restrict__ seed, uint32_t thr, float scale,
               T* __restrict__ r_out, T* __restrict__ normed,
               float* __restrict__ mean_out, float* __restrict__ rstd_out,
               int64_t n_rows, int D, float eps) {
  const int wave = threadIdx.x / DR_WAVE;
  const int lane = threadIdx.x % DR_WAVE;
  const int waves_per_block = blockDim.x / DR_WAVE;
  const int64_t row0 = (int64_t)blockIdx.x * waves_per_block + wave;
  const int64_t stride_rows = (int64_t)gridDim.x * waves_per_block;
  PhiloxKey pk = {0u, 0u, 0u, 0u};
  if (HAS_MASK) pk = philox_key(seed);

  for (int64_t row = row0; row < n_rows; row += stride_rows) {
    const int64_t base = row * D;
    float v[MAX_PER_LANE];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAX_PER_LANE; ++i) {
      v[i] = 0.f;
      if (i * DR_WAVE >= D) break;
      const int j = lane + i * DR_WAVE;
      if (j < D) {
        const float a = HAS_ADD ? ldf(branch + base + j) : 0.f;
        float r = ldf(residual + base + j);
        if (HAS_ADD) {
          if (HAS_MASK)
            r += philox_keep1((uint64_t)(base + j), pk, thr) ? a * scale : 0.f;
          else
            r += a;
          r = round_io<T>(r);
          stf(r_out + base + j, r);
        }
        v[i] = r;
        s += r;
      }
    }
    if (HAS_NORM) {
      s = wave_sum(s);
      const float mean = s / D;
      float var = 0.f;
#pragma unroll
      for (int i = 0; i < MAX_PER_LANE; ++i) {
        if (i * DR_WAVE >= D) break;
        if (lane + i * DR_WAVE < D) { float d = v[i] - mean; var += d * d; }
      }
      var = wave_sum(var) / D;
      const float rstd = rsqrtf(var + eps);
      if (lane == 0) {
        mean_out[row] = mean;
        rstd_out[row] = rstd;
      }
#pragma unroll
      for (int i = 0; i < MAX_PER_LANE; ++i) {
        if (i * DR_WAVE >= D) break;
        const int j = lane + i * DR_WAVE;
        if (j < D) stf(normed + base + j, (v[i] - mean) * rstd * w[j] + b[j]);
      }
    }
  }
}

// D > 1024: nothing is held per lane.  Each lane re-reads the r_out values it
// has just stored (same thread, same address: program order makes them
// visible; they come back from L1/L2), so any D runs without scratch.
// HAS_ADD off stores no r_out and re-reads the input row itself.
template <typename T, bool HAS_ADD, bool HAS_MASK, bool HAS_NORM>
__global__ void __launch_bounds__(256)
dal_fwd_stream(const T* __restrict__ branch, const T* __restrict__ residual,
               const float* __restrict__ w, const float* __restrict__ b,
               const int64_t* __restrict__ seed, uint32_t thr, float scale,
               T* r_out, T* __restrict__ normed,
               float* __restrict__ mean_out, float* __restrict__ rstd_out,
               int64_t n_rows, int D, float eps) {
  const int wave = threadIdx.x / DR_WAVE;
  const int lane = threadIdx.x % DR_WAVE;
  const int waves_per_block = blockDim.x / DR_WAVE;
  const int64_t row0 = (int64_t)blockIdx.x * waves_per_block + wave;
  const int64_t stride_rows = (int64_t)gridDim.x * waves_per_block;
  PhiloxKey pk = {0u, 0u, 0u, 0u};
  if (HAS_MASK) pk = philox_key(seed);

  for (int64_t row = row0; row < n_rows; row += stride_rows) {
    const int64_t base = row * D;
    float s = 0.f;
    for (int j = lane; j < D; j += DR_WAVE) {
      const float a = HAS_ADD ? ldf(branch + base + j) : 0.f;
      float r = ldf(residual + base + j);
      if (HAS_ADD) {
        if (HAS_MASK)
          r += philox_keep1((uint64_t)(base + j), pk, thr) ? a * scale : 0.f;
        else
          r += a;
        r = round_io<T>(r);
        stf(r_out + base + j, r);
      }
      s += r;
    }
    if (HAS_NORM) {
      const T* x = HAS_ADD ? r_out : residual;  // the row the stats are over
      s = wave_sum(s);
      const float mean = s / D;
      float var = 0.f;
      for (int j = lane; j < D; j += DR_WAVE) {
        float d = ldf(x + base + j) - mean;
        var += d * d;
      }
      var = wave_sum(var) / D;
      const float rstd = rsqrtf(var + eps);
      if (lane == 0) {
        mean_out[row] = mean;
        rstd_out[row] = rstd;
      }
      for (int j = lane; j < D; j += DR_WAVE)
        stf(normed + base + j, (ldf(x + base + j) - mean) * rstd * w[j] + b[j]);
    }
  }
}

// ----------------------------------------------------------------- backward
//   d_total    = LN-backward(d_normed; r_out) + d_r_out
//   d_residual = d_total
//   d_branch   = d_total * keep / (1 - p)      (mask regenerated)
// d_res is written only with HAS_NORM (otherwise d_residual IS d_r_out) and
// d_branch only with HAS_MASK (otherwise it equals d_residual).
// HAS_ADD off: r_out is the op's x, d_r_out is not read and d_res is dx.
// vec4 dw/db: the lane owns the same columns in every row, so they accumulate
// in registers across the row loop (no atomics in it); one LDS combine per
// block, then a (gridDim.x, 2, D) partial slab that the host sums.
template <typename T, bool HAS_ADD, bool HAS_MASK, bool HAS_NORM>
__global__ void __launch_bounds__(256)
dal_bwd_vec4(const T* __restrict__ d_normed, const T* __restrict__ d_r_out,
             const T* __restrict__ r_out, const float* __restrict__ w,
             const float* __restrict__ mean, const float* __restrict__ rstd,
             const int64_t* __restrict__ seed, uint32_t thr, float scale,
             T* __restrict__ d_res, T* __restrict__ d_branch,
             float* __restrict__ dwdb_part, int64_t n_rows, int D) {
  extern __shared__ float smem[];  // HAS_NORM: 2 * D floats [dw | db]
  float* dw_s = smem;
  float* db_s = smem + D;
  if (HAS_NORM) {
    for (int j = threadIdx.x; j < 2 * D; j += blockDim.x) smem[j] = 0.f;
    __syncthreads();
  }

  const int wave = threadIdx.x / DR_WAVE;
  const int lane = threadIdx.x % DR_WAVE;
  const int waves_per_block = blockDim.x / DR_WAVE;
  const int64_t row0 = (int64_t)blockIdx.x * waves_per_block + wave;
  const int64_t stride_rows = (int64_t)gridDim.x * waves_per_block;
  const int j0 = lane * 4;
  const bool active = j0 < D;
  const float invD = 1.f / D;
  float wr[4] = {0.f, 0.f, 0.f, 0.f};
  if (HAS_NORM && active) ld4(w + j0, wr);
  float dwacc[4] = {0.f, 0.f, 0.f, 0.f}, dbacc[4] = {0.f, 0.f, 0.f, 0.f};
  PhiloxKey pk = {0u, 0u, 0u, 0u};
  if (HAS_MASK) pk = philox_key(seed);

  for (int64_t row = row0; row < n_rows; row += stride_rows) {
    const int64_t off = row * D + j0;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    if (HAS_ADD && active) ld4(d_r_out + off, t);
    if (HAS_NORM) {
      float g[4] = {0.f, 0.f, 0.f, 0.f}, xv[4] = {0.f, 0.f, 0.f, 0.f};
      if (active) {
        ld4(d_normed + off, g);
        ld4(r_out + off, xv);
      }
      const float mu = mean[row];
      const float rs = rstd[row];
      float xh[4], gw[4];
      float a = 0.f, bsum = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xh[i] = (xv[i] - mu) * rs;
        gw[i] = g[i] * wr[i];
        a += gw[i] * xh[i];
        bsum += gw[i];
      }
      a = wave_sum(a) * invD;
      bsum = wave_sum(bsum) * invD;
      if (active) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float dx = rs * (gw[i] - bsum - xh[i] * a);
          t[i] = HAS_ADD ? t[i] + dx : dx;
          dwacc[i] += g[i] * xh[i];
          dbacc[i] += g[i];
        }
        st4(d_res + off, t);
      }
    }
    if (HAS_MASK && active) {
      uint32_t o[4];
      philox4((uint64_t)off >> 2, pk, o);
      float u[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) u[i] = (o[i] >= thr) ? t[i] * scale : 0.f;
      st4(d_branch + off, u);
    }
  }
  if (HAS_NORM) {
    if (active) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        atomicAdd(&dw_s[j0 + i], dwacc[i]);
        atomicAdd(&db_s[j0 + i], dbacc[i]);
      }
    }
    __syncthreads();
    float* out = dwdb_part + (int64_t)blockIdx.x * 2 * D;
    for (int j = threadIdx.x; j < 2 * D; j += blockDim.x) out[j] = smem[j];
  }
}

template <typename T, int MAX_PER_LANE, bool HAS_ADD, bool HAS_MASK, bool HAS_NORM>
__global__ void __launch_bounds__(256)
dal_bwd_kernel(const T* __restrict__ d_normed, const T* __restrict__ d_r_out,
               const T* __restrict__ r_out, const float* __restrict__ w,
               const float* __restrict__ mean, const float* __restrict__ rstd,
               const int64_t* __restrict__ seed, uint32_t thr, float scale,
               T* __restrict__ d_res, T* __restrict__ d_branch,
               float* __restrict__ dwdb_part, int64_t n_rows, int D) {
  extern __shared__ float smem[];  // HAS_NORM: 2 * D floats [dw | db]
  float* dw_s = smem;
  float* db_s = smem + D;
  if (HAS_NORM) {
    for (int j = threadIdx.x; j < 2 * D; j += blockDim.x) smem[j] = 0.f;
    __syncthreads();
  }

  const int wave = threadIdx.x / DR_WAVE;
  const int lane = threadIdx.x % DR_WAVE;
  const int waves_per_block = blockDim.x / DR_WAVE;
  const int64_t row0 = (int64_t)blockIdx.x * waves_per_block + wave;
  const int64_t stride_rows = (int64_t)gridDim.x * waves_per_block;
  PhiloxKey pk = {0u, 0u, 0u, 0u};
  if (HAS_MASK) pk = philox_key(seed);

  for (int64_t row = row0; row < n_rows; row += stride_rows) {
    const int64_t base = row * D;
    float gy[MAX_PER_LANE], xh[MAX_PER_LANE];
    float mu = 0.f, rs = 0.f, a = 0.f, bsum = 0.f;
    if (HAS_NORM) {
      mu = mean[row];
      rs = rstd[row];
#pragma unroll
      for (int i = 0; i < MAX_PER_LANE; ++i) {
        gy[i] = 0.f;
        xh[i] = 0.f;
        if (i * DR_WAVE >= D) break;
        const int j = lane + i * DR_WAVE;
        if (j < D) {
          const float g = ldf(d_normed + base + j);
          const float h = (ldf(r_out + base + j) - mu) * rs;
          const float gw = g * w[j];
          gy[i] = gw;
          xh[i] = h;
          a += gw * h;
          bsum += gw;
        }
      }
      a = wave_sum(a) / D;
      bsum = wave_sum(bsum) / D;
    }
#pragma unroll
    for (int i = 0; i < MAX_PER_LANE; ++i) {
      if (i * DR_WAVE >= D) break;
      const int j = lane + i * DR_WAVE;
      if (j < D) {
        float t = HAS_ADD ? ldf(d_r_out + base + j) : 0.f;
        if (HAS_NORM) {
          const float dx = rs * (gy[i] - bsum - xh[i] * a);
          t = HAS_ADD ? t + dx : dx;
          stf(d_res + base + j, t);
          const float g = ldf(d_normed + base + j);
          atomicAdd(&dw_s[j], g * xh[i]);
          atomicAdd(&db_s[j], g);
        }
        if (HAS_MASK)
          stf(d_branch + base + j,
              philox_keep1((uint64_t)(base + j), pk, thr) ? t * scale : 0.f);
      }
    }
  }
  if (HAS_NORM) {
    __syncthreads();
    float* out = dwdb_part + (int64_t)blockIdx.x * 2 * D;
    for (int j = threadIdx.x; j < 2 * D; j += blockDim.x) out[j] = smem[j];
  }
}

// D > 1024: two passes over the row, nothing held per lane (see dal_fwd_stream)
template <typename T, bool HAS_ADD, bool HAS_MASK, bool HAS_NORM>
__global__ void __launch_bounds__(256)
dal_bwd_stream(const T* __restrict__ d_normed, const T* __restrict__ d_r_out,
               const T* __restrict__ r_out, const float* __restrict__ w,
               const float* __restrict__ mean, const float* __restrict__ rstd,
               const int64_t* __restrict__ seed, uint32_t thr, float scale,
               T* __restrict__ d_res, T* __restrict__ d_branch,
               float* __restrict__ dwdb_part, int64_t n_rows, int D) {
  extern __shared__ float smem[];  // HAS_NORM: 2 * D floats [dw | db]
  float* dw_s = smem;
  float* db_s = smem + D;
  if (HAS_NORM) {
    for (int j = threadIdx.x; j < 2 * D; j += blockDim.x) smem[j] = 0.f;
    __syncthreads();
  }

  const int wave = threadIdx.x / DR_WAVE;
  const int lane = threadIdx.x % DR_WAVE;
  const int waves_per_block = blockDim.x / DR_WAVE;
  const int64_t row0 = (int64_t)blockIdx.x * waves_per_block + wave;
  const int64_t stride_rows = (int64_t)gridDim.x * waves_per_block;
  PhiloxKey pk = {0u, 0u, 0u, 0u};
  if (HAS_MASK) pk = philox_key(seed);

  for (int64_t row = row0; row < n_rows; row += stride_rows) {
    const int64_t base = row * D;
    float mu = 0.f, rs = 0.f, a = 0.f, bsum = 0.f;
    if (HAS_NORM) {
      mu = mean[row];
      rs = rstd[row];
      for (int j = lane; j < D; j += DR_WAVE) {
        const float gw = ldf(d_normed + base + j) * w[j];
        a += gw * ((ldf(r_out + base + j) - mu) * rs);
        bsum += gw;
      }
      a = wave_sum(a) / D;
      bsum = wave_sum(bsum) / D;
    }
    for (int j = lane; j < D; j += DR_WAVE) {
      float t = HAS_ADD ? ldf(d_r_out + base + j) : 0.f;
      if (HAS_NORM) {
        const float g = ldf(d_normed + base + j);
        const float h = (ldf(r_out + base + j) - mu) * rs;
        const float dx = rs * (g * w[j] - bsum - h * a);
        t = HAS_ADD ? t + dx : dx;
        stf(d_res + base + j, t);
        atomicAdd(&dw_s[j], g * h);
        atomicAdd(&db_s[j], g);
      }
      if (HAS_MASK)
        stf(d_branch + base + j,
            philox_keep1((uint64_t)(base + j), pk, thr) ? t * scale : 0.f);
    }
  }
  if (HAS_NORM) {
    __syncthreads();
    float* out = dwdb_part + (int64_t)blockIdx.x * 2 * D;
    for (int j = threadIdx.x; j < 2 * D; j += blockDim.x) out[j] = smem[j];
  }
}

// ---------------------------------------------------------------- launchers
// D picks the kernel: vec4, 4 or 16 values per lane, or the streaming body.
template <typename T, bool HAS_ADD, bool HAS_MASK, bool HAS_NORM>
static hipError_t dal_fwd_launch(const void* branch, const void* residual,
                                 const float* w, const float* b,
                                 const int64_t* seed, uint32_t thr, float scale,
                                 void* r_out, void* normed, float* mean,
                                 float* rstd, int64_t n_rows, int D, float eps,
                                 hipStream_t stream) {
  const int block = 256;
  const int waves = block / DR_WAVE;
  int grid = (int)std::min<int64_t>((n_rows + waves - 1) / waves, 2048);
  if (grid == 0) grid = 1;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream,
                       (const T*)branch, (const T*)residual, w, b, seed, thr,
                       scale, (T*)r_out, (T*)normed, mean, rstd, n_rows, D, eps);
    return hipGetLastError();
  };
  if ((D % 4) == 0 && D <= 4 * DR_WAVE)
    return launch(dal_fwd_vec4<T, HAS_ADD, HAS_MASK, HAS_NORM>);
  if (D <= 256) return launch(dal_fwd_kernel<T, 4, HAS_ADD, HAS_MASK, HAS_NORM>);
  if (D <= 1024) return launch(dal_fwd_kernel<T, 16, HAS_ADD, HAS_MASK, HAS_NORM>);
  return launch(dal_fwd_stream<T, HAS_ADD, HAS_MASK, HAS_NORM>);
}

template <typename T, bool HAS_ADD, bool HAS_MASK, bool HAS_NORM>
static hipError_t dal_bwd_launch(const void* d_normed, const void* d_r_out,
                                 const void* r_out, const float* w,
                                 const float* mean, const float* rstd,
                                 const int64_t* seed, uint32_t thr, float scale,
                                 void* d_res, void* d_branch, float* dwdb_part,
                                 int n_blocks, int64_t n_rows, int D,
                                 hipStream_t stream) {
  const int block = 256;
  const size_t smem = HAS_NORM ? 2 * D * sizeof(float) : 0;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(block), smem, stream,
                       (const T*)d_normed, (const T*)d_r_out, (const T*)r_out, w,
                       mean, rstd, seed, thr, scale, (T*)d_res, (T*)d_branch,
                       dwdb_part, n_rows, D);
    return hipGetLastError();
  };
  if ((D % 4) == 0 && D <= 4 * DR_WAVE)
    return launch(dal_bwd_vec4<T, HAS_ADD, HAS_MASK, HAS_NORM>);
  if (D <= 256) return launch(dal_bwd_kernel<T, 4, HAS_ADD, HAS_MASK, HAS_NORM>);
  if (D <= 1024) return launch(dal_bwd_kernel<T, 16, HAS_ADD, HAS_MASK, HAS_NORM>);
  return launch(dal_bwd_stream<T, HAS_ADD, HAS_MASK, HAS_NORM>);
}

constexpr std::true_type on{};
constexpr std::false_type off{};

}  // namespace dr

// Entry contracts: kernels.h.  The ladders below name every (HAS_ADD,
// HAS_MASK, HAS_NORM) instance that exists.
extern "C" {

int dr_dropout_add_ln_fwd(const void* branch, const void* residual, const float* w,
                          const float* b, const int64_t* seed, uint32_t thr,
                          float scale, void* r_out, void* normed, float* mean,
                          float* rstd, int64_t n_rows, int D, float eps,
                          int is_bf16, hipStream_t stream) {
  const bool a = branch != nullptr, m = seed != nullptr, n = w != nullptr;
  return (int)dr::with_io_type(is_bf16, [&](auto io) {
    auto go = [&](auto A, auto M, auto N) {
      return dr::dal_fwd_launch<typename decltype(io)::type, decltype(A)::value,
                                decltype(M)::value, decltype(N)::value>(
          branch, residual, w, b, seed, thr, scale, r_out, normed, mean, rstd,
          n_rows, D, eps, stream);
    };
    using dr::on, dr::off;
    if (!a) return go(off, off, on);
    if (m) return n ? go(on, on, on) : go(on, on, off);
    return n ? go(on, off, on) : go(on, off, off);
  });
}

int dr_dropout_add_ln_bwd(const void* d_normed, const void* d_r_out,
                          const void* r_out, const float* w, const float* mean,
                          const float* rstd, const int64_t* seed, uint32_t thr,
                          float scale, void* d_res, void* d_branch,
                          float* dwdb_part, int n_blocks, int64_t n_rows, int D,
                          int is_bf16, hipStream_t stream) {
  const bool a = d_r_out != nullptr, m = seed != nullptr, n = w != nullptr;
  return (int)dr::with_io_type(is_bf16, [&](auto io) {
    auto go = [&](auto A, auto M, auto N) {
      return dr::dal_bwd_launch<typename decltype(io)::type, decltype(A)::value,
                                decltype(M)::value, decltype(N)::value>(
          d_normed, d_r_out, r_out, w, mean, rstd, seed, thr, scale, d_res,
          d_branch, dwdb_part, n_blocks, n_rows, D, stream);
    };
    using dr::on, dr::off;
    if (!a) return go(off, off, on);
    if (m) return n ? go(on, on, on) : go(on, on, off);
    // no mask and no norm: nothing to launch (there is no such instance)
    return n ? go(on, off, on) : hipSuccess;
  });
}

}  // extern "C"
