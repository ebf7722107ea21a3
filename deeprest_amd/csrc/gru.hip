// Fused GRU sequence kernel for gfx950 — the framework's hot op.
//
// Replaces the reference's cuDNN GRU (reference: resource-estimation/
// qrnn.py:24,41) with an MI355X-native design: the WHOLE sequence runs in one
// kernel launch.  Rows (= batch x component pairs) evolve independently, so
// each 4-wave workgroup owns a 64-row tile, stages the recurrent weight
// matrix W_hh (3H x H bf16 = 96 KB) in XOR-swizzled LDS once, keeps its
// rows' fp32 hidden state entirely in registers, and per time step runs a
// 64x384x128 MFMA GEMM (v_mfma_f32_16x16x32_bf16) fused with the
// sigmoid/tanh gate epilogue and the per-component FiLM conditioning
// (g = xg * gamma + beta).  State stays fp32; GEMM operands are bf16
// (SURVEY.md "keep state in fp32, activations in low precision").
//
// IO layout note: the training-only side tensors (forward saves r|z,
// backward dpre dr|dz|d_hhn|dn) use a within-row permutation "pi":
//   pi(gate, col) = gate*H + (col & 15)*8 + (col >> 4)
// so each lane's 8 values per gate (its MFMA C-fragment columns, stride 16)
// are CONTIGUOUS 16 bytes -> one vector load/store instead of 8 scalars.
// Only this file and ops/gru.py (the dW row unpermute) know about pi.
//
// Backward: the sequential chain only — per reversed step compute the gate
// pre-activation grads (phase A, vectorized pi IO) and the recurrent term
// dh_prev = dh*z + dpre @ W_hh.  The dpre tile round-trips through L2 (same
// CU writes then reads it after __syncthreads; per-CU L1 is updated by its
// own stores), against a pi-row-permuted W image in LDS, so no LDS dpre
// image and one barrier per step.  Batched reductions (dW_hh, db_hh, dgamma,
// dbeta, dx_gates) happen outside: one rocBLAS GEMM over dpre's first three
// slices (the MFMA K axis below, which is why d_hhn sits before dn) + the
// reduce kernels below (driven by ops/gru.py).
//
// Fixed geometry: H = 128, 3H = 384, 64 rows/block, 4 waves, 256 threads.
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace dr {

constexpr int H = 128;        // hidden size (fixed)
constexpr int G3H = 384;      // 3*H
constexpr int G4H = 512;      // 4*H
constexpr int ROWS = 64;      // rows per block
constexpr int WAVES = 4;
constexpr int THREADS = WAVES * DR_WAVE;
constexpr int KT = H / 32;    // K-tiles of 32 in the fwd GEMM (4)
constexpr int NT = G3H / 16;  // N-tiles of 16 (24)
constexpr int XG_SLOTS = 32;  // xg staging slots: waves x batches a wave's 16 rows span

constexpr int LDS_MAX = 163840;  // dynamic LDS one workgroup may declare

// Dynamic-LDS layout of gru_fwd_kernel<., ., FP8, NSUB, HEADS> (one region,
// every offset 16 B aligned): the kernel takes its pointers from it and the
// launcher its size.
// Forward stages W in LDS (an L2-streamed W was measured SLOWER for the
// forward: 96 KB/wave/step of L2 B-fragment traffic outweighed the
// occupancy gain).
template <bool FP8, int NSUB, bool HEADS>
struct FwdLds {
  static constexpr int ELT = FP8 ? 1 : 2;                  // GEMM-tile element bytes
  static constexpr int W = 0;                              // 384 x 128 swizzled
  static constexpr int WH = W + G3H * H * ELT;             // (HEADS) 32 x 128 bf16 swizzled
  static constexpr int HM = WH + (HEADS ? 32 * H * 2 : 0); // h mirror, ROWS*NSUB x 128 swizzled
  static constexpr int XG = HM + ROWS * NSUB * H * ELT;    // 32 x 384 bf16, pi layout
  static constexpr int TOTAL = XG + XG_SLOTS * G3H * 2;
  static_assert(TOTAL <= LDS_MAX, "forward LDS layout exceeds a workgroup's LDS");
};

// Same for gru_bwd_kernel<., NSUB, FUSED>.  NSUB == 1 uses NO LDS: the
// pi-permuted W image stays in L2 (96 KB, shared by every block) so occupancy
// is VGPR-bound (2-3 waves/SIMD) instead of LDS-bound (1 wave/SIMD) — the
// kernel is latency-bound, occupancy hides it.
template <int NSUB, bool FUSED>
struct BwdLds {
  static constexpr int W = 0;                    // 128 x 384 bf16, swz768 rows
  static constexpr int WN = W + H * G3H * 2;     // 128 x 128 bf16 swizzled
  static constexpr int WH = WN + H * H * 2;      // (FUSED) 128 x 32 bf16 linear
  static constexpr int TOTAL = NSUB == 2 ? WH + (FUSED ? H * 32 * 2 : 0) : 0;
  static_assert(TOTAL <= LDS_MAX, "backward LDS layout exceeds a workgroup's LDS");
};

// swizzled byte address inside a row-major [rows][128] bf16 tile (256 B rows)
__device__ __forceinline__ int swz(int row, int k_elem) {
  int blk = k_elem >> 3;            // 8 bf16 = 16 B per block
  int within = (k_elem & 7) * 2;
  return row * 256 + ((blk ^ (row & 15)) << 4) + within;
}

// same for a row-major [rows][128] fp8 tile (128 B rows, 8 B blocks)
__device__ __forceinline__ int swz8(int row, int k_elem) {
  int blk = k_elem >> 3;
  return row * 128 + ((blk ^ (row & 15)) << 3) + (k_elem & 7);
}

__device__ __forceinline__ uint8_t f2fp8(float v) {
  __hip_fp8_e4m3 x(v);              // OCP e4m3fn on gfx950 (hardware cvt)
  return x.__x;
}

// same swizzle for a row-major [rows][384] bf16 tile (768 B rows)
__device__ __forceinline__ int swz768(int row, int k_elem) {
  int blk = k_elem >> 3;
  int within = (k_elem & 7) * 2;
  return row * 768 + ((blk ^ (row & 15)) << 4) + within;
}

__device__ __forceinline__ bf16x8 lds_read8(const char* base, int byte_off) {
  return *reinterpret_cast<const bf16x8*>(base + byte_off);
}

// Orders ONE wave's own LDS accesses: what some lanes wrote before it, other
// lanes of the same wave may read after it.  The hardware executes a wave's
// LDS operations in issue order, so a wavefront-scope fence costs no
// instruction and no wait; it only pins the compiler's ordering.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- pi-layout vector IO: 8 lane-owned values <-> 16/32 contiguous bytes ----
template <typename T>
__device__ __forceinline__ void st8(T* dst, const float* v);
template <>
__device__ __forceinline__ void st8<uint16_t>(uint16_t* dst, const float* v) {
  uint4 p;
  p.x = f2bf2(v[0], v[1]);
  p.y = f2bf2(v[2], v[3]);
  p.z = f2bf2(v[4], v[5]);
  p.w = f2bf2(v[6], v[7]);
  *reinterpret_cast<uint4*>(dst) = p;
}
template <>
__device__ __forceinline__ void st8<float>(float* dst, const float* v) {
  *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(v);
  *reinterpret_cast<float4*>(dst + 4) = *reinterpret_cast<const float4*>(v + 4);
}

template <typename T>
__device__ __forceinline__ void ld8(const T* src, float* v);
template <>
__device__ __forceinline__ void ld8<uint16_t>(const uint16_t* src, float* v) {
  uint4 raw = *reinterpret_cast<const uint4*>(src);
  const uint16_t* p = reinterpret_cast<const uint16_t*>(&raw);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = bf2f(p[e]);
}
template <>
__device__ __forceinline__ void ld8<float>(const float* src, float* v) {
  *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(src);
  *reinterpret_cast<float4*>(v + 4) = *reinterpret_cast<const float4*>(src + 4);
}

// 8 IO values as loaded, bf16 (4 registers) or f32 (8), widened where used
template <typename T> struct Raw8;
template <> struct Raw8<uint16_t> { uint4 v; };
template <> struct Raw8<float> { float4 a, b; };
__device__ __forceinline__ void widen8(const Raw8<uint16_t>& p, float* v) {
  const uint32_t w[4] = {p.v.x, p.v.y, p.v.z, p.v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void widen8(const Raw8<float>& p, float* v) {
  v[0] = p.a.x; v[1] = p.a.y; v[2] = p.a.z; v[3] = p.a.w;
  v[4] = p.b.x; v[5] = p.b.y; v[6] = p.b.z; v[7] = p.b.w;
}
// 8 values at a 32-bit BYTE offset from a kernel-argument pointer.  The base
// stays a uniform global pointer and the offset one VGPR, so the load is a
// global_load_dwordx4 with a scalar base; an opaque POINTER would lose its
// address space and come out as flat loads behind 64-bit vector adds.
template <typename T>
__device__ __forceinline__ Raw8<T> ld_raw_at(const T* base, uint32_t byte_off);
template <>
__device__ __forceinline__ Raw8<uint16_t> ld_raw_at<uint16_t>(const uint16_t* base,
                                                              uint32_t byte_off) {
  return {*reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(base) + byte_off)};
}
template <>
__device__ __forceinline__ Raw8<float> ld_raw_at<float>(const float* base,
                                                        uint32_t byte_off) {
  const char* p = reinterpret_cast<const char*>(base) + byte_off;
  return {*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 16)};
}
// A product rounded on its own, whatever -ffp-contract allows around it
// (__fmul_rn is a plain multiply here and gets contracted like one).
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
// A zero the optimizer cannot see through.  Added to the offset of a
// t-invariant operand inside the time loop it keeps the loads in the loop
// (hoisted they would take registers the streaming variants do not have).
__device__ __forceinline__ uint32_t opaque_zero() {
  uint32_t z = 0;
  asm volatile("" : "+v"(z));
  return z;
}

// store an 8-wide bf16 fragment to a T-typed tensor (bf16: one 16 B store)
template <typename T>
__device__ __forceinline__ void st_frag(T* dst, bf16x8 v);
template <>
__device__ __forceinline__ void st_frag<uint16_t>(uint16_t* dst, bf16x8 v) {
  *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&v);
}
template <>
__device__ __forceinline__ void st_frag<float>(float* dst, bf16x8 v) {
  const uint16_t* p = reinterpret_cast<const uint16_t*>(&v);
#pragma unroll
  for (int e = 0; e < 8; ++e) dst[e] = bf2f(p[e]);
}

// load 8 T values as raw bf16 bit patterns (bf16: one 16 B load)
template <typename T>
__device__ __forceinline__ void ld_raw8(const T* src, uint16_t* out);
template <>
__device__ __forceinline__ void ld_raw8<uint16_t>(const uint16_t* src, uint16_t* out) {
  uint4 raw = *reinterpret_cast<const uint4*>(src);
  *reinterpret_cast<uint4*>(out) = raw;
}
template <>
__device__ __forceinline__ void ld_raw8<float>(const float* src, uint16_t* out) {
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = f2bf(src[e]);
}

// load 8 values directly as an MFMA bf16 fragment (no f32 round trip)
template <typename T>
__device__ __forceinline__ bf16x8 ld_frag(const T* src);
template <>
__device__ __forceinline__ bf16x8 ld_frag<uint16_t>(const uint16_t* src) {
  return *reinterpret_cast<const bf16x8*>(src);
}
template <>
__device__ __forceinline__ bf16x8 ld_frag<float>(const float* src) {
  uint16_t p[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) p[e] = f2bf(src[e]);
  return *reinterpret_cast<bf16x8*>(p);
}

// ---------------------------------------------------------------- forward
// FP8 = true: W and the h mirror live in LDS as OCP e4m3 and the recurrent
// GEMM runs on v_mfma_f32_16x16x32_fp8_fp8 (state stays fp32 in registers;
// activations/outputs keep dtype T).  Inference-only (BASELINE config 5:
// fp8 MFMA for the long-horizon path); training uses bf16.
// NSUB = 2: 8 waves / 128-row tile — 2 waves/SIMD (the kernel is
// latency-stalled at 1 wave/SIMD); gamma/beta/b_hh then stream from L1/L2
// instead of registers so each wave fits the 256-reg budget.
// Wave ownership: a wave's A-fragments, epilogue, head phase and h_all store
// touch only its own 16 rows of the h mirror, and it stages x_gates for the
// batches of those rows into its own slots of the XG region.  After the
// prologue the waves of a block share nothing they write, so the time loop
// has no workgroup barrier and the waves free-run (as in the backward).
// HEADS = true: after each step's epilogue every wave multiplies its own 16
// rows of the h mirror by the quantile heads' weight image wh_fwd (32, H)
// bf16 — wh_fwd[o][k] = w_head[o][k], exact zero rows for o >= O — on two
// more 16-wide N-tiles and stores out (B, TT, C, O).  The image sits in LDS as
// 32 more 256-byte rows behind the W image (8 KB, same swizzle, whatever FP8
// is).  Inference decode (SAVE = false): h_all is never written and the state
// after the last processed step goes to h_last (B, C, H).  Training forward
// (SAVE = true, 8-wave tile only): saves, out and h_all are all written, and
// there is no h_last.
// VARLEN = true (HEADS only): batch b is valid at t < clamp(lens[b], 1, TT).
// A row whose time index is padding HOLDS its state through a select on
// hnew — whatever the padded xg holds, NaN included, is computed and thrown
// away — rewrites the identical rounded value into the h mirror, and stores
// no head output (out arrives zeroed).  Rows of one wave differ in length,
// so the predicate is per row; each lane keeps its 4 rows' clamped lengths
// in registers (the 8-wave variant has no LDS byte left).  The FP8 variant
// already fills all 512 registers and spills, so its lengths twin streams
// gamma / beta / b_hh from L1/L2 per step, as the 8-wave variant does,
// instead of holding them in 120 registers — gamma / beta rounded to bf16 on
// the way, so the values are the ones the packed registers hold.  h_last is
// each row's state after its own last valid step.
// Whether a forward variant holds gamma / beta / b_hh in registers.  The
// others stream them per step from the pi-ordered operand images (see
// gru_operand_images_kernel), which their launcher builds first.
template <bool FP8, int NSUB, bool VARLEN>
constexpr bool fwd_gb_regs = (NSUB == 1) && !(VARLEN && FP8);

template <typename T, bool SAVE, bool FP8 = false, int NSUB = 1, bool HEADS = false,
          bool VARLEN = false>
__global__ __launch_bounds__(THREADS * NSUB) void gru_fwd_kernel(
    const T* __restrict__ xg,      // (B, TT, 3H)
    const T* __restrict__ gamma,   // (C, 3H); the streaming variants (!GB_REGS)
    const T* __restrict__ beta,    // (C, 3H)  take the pi-ordered operand
    const uint16_t* __restrict__ w_gemm,  // (3H, H) bf16 GEMM weight image
    const float* __restrict__ b_hh,  // (3H,)  images of these three instead
    const T* __restrict__ h0,      // (B, C, H)
    T* __restrict__ h_all,         // (B, TT, C, H)
    T* __restrict__ saves,         // (B, TT, C, 4H) pi layout (SAVE only)
    int B, int TT, int C, int reverse,
    const uint16_t* __restrict__ wh_fwd,  // HEADS: (32, H) bf16 head weight image
    T* __restrict__ out,           // HEADS: (B, TT, C, O)
    T* __restrict__ h_last,        // HEADS: (B, C, H)
    int O,
    const int* __restrict__ lens) {  // VARLEN: (B,) int32
  static_assert(HEADS || !VARLEN, "per-row lengths exist in the decode kernel only");
  static_assert(!(SAVE && (VARLEN || FP8)),
                "the saving kernels run full windows on bf16 GEMM tiles");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using L = FwdLds<FP8, NSUB, HEADS>;
  constexpr int BROWS = ROWS * NSUB;           // rows per block
  constexpr int BTHREADS = THREADS * NSUB;
  char* Wl = smem + L::W;
  char* WHl = smem + L::WH;
  char* Hl = smem + L::HM;
  char* XGl = smem + L::XG;
  // gamma/beta/b_hh in registers (NSUB == 1) or streamed per step
  constexpr bool GB_REGS = fwd_gb_regs<FP8, NSUB, VARLEN>;

  const int tid = threadIdx.x;
  const int wv = tid / DR_WAVE;
  const int lane = tid % DR_WAVE;
  const int64_t R = (int64_t)B * C;
  const int64_t r0 = (int64_t)blockIdx.x * BROWS;

  // ---- prologue: stage the W image into swizzled LDS ----
  for (int id = tid; id < G3H * (H / 8); id += BTHREADS) {
    int j = id / (H / 8);
    int blk = id % (H / 8);
    bf16x8 v = *reinterpret_cast<const bf16x8*>(w_gemm + (int64_t)j * H + blk * 8);
    if constexpr (FP8) {
      const uint16_t* bv = reinterpret_cast<const uint16_t*>(&v);
      uint8_t q[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) q[e] = f2fp8(bf2f(bv[e]));
      *reinterpret_cast<uint64_t*>(Wl + j * 128 + ((blk ^ (j & 15)) << 3)) =
          *reinterpret_cast<const uint64_t*>(q);
    } else {
      *reinterpret_cast<bf16x8*>(Wl + j * 256 + ((blk ^ (j & 15)) << 4)) = v;
    }
  }
  if constexpr (HEADS) {
    for (int id = tid; id < 32 * (H / 8); id += BTHREADS) {
      int j = id / (H / 8);
      int blk = id % (H / 8);
      *reinterpret_cast<bf16x8*>(WHl + j * 256 + ((blk ^ (j & 15)) << 4)) =
          *reinterpret_cast<const bf16x8*>(wh_fwd + j * H + blk * 8);
    }
  }

  // ---- per-lane static geometry (C-layout of the 16x16 MFMA tile) ----
  const int c_col = lane & 15;           // col within a 16-wide N-tile
  const int rgrp = lane >> 4;            // row group (0..3)
  int row_of[4];
  int64_t r_abs[4];
  int b_of[4], comp_of[4];
  bool live[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    row_of[i] = wv * 16 + rgrp * 4 + i;
    r_abs[i] = r0 + row_of[i];
    live[i] = r_abs[i] < R;
    int64_t rr = live[i] ? r_abs[i] : (R - 1);
    b_of[i] = (int)(rr / C);
    comp_of[i] = (int)(rr % C);
  }
  // VARLEN: this lane's rows' lengths, clamped here so that no value can
  // index outside [0, TT)
  int len_of[4];
  if constexpr (VARLEN) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      len_of[i] = std::min(std::max(lens[b_of[i]], 1), TT);
    }
  }

  // ---- preload T-invariant per-lane values ----
  // NSUB==1: gamma/beta packed as bf16 pairs in one u32 per (row, gate,
  // tile) — LDS caps this variant at 1 block/CU so the registers are free.
  // NSUB==2: two waves/SIMD need the registers back; gamma/beta/b_hh are
  // L1/L2-resident and reload per step from the pi-ordered images, where a
  // lane's 8 values of one (row, gate) are one 16-byte load (f32: two).
  constexpr int GBN = GB_REGS ? 8 : 1;
  uint32_t gb[4][3][GBN];
  float bh[3][GBN];
  int gb_off[4];            // GB_REGS: element offset of the row's component
  uint32_t gbi_off[4];      // streaming: byte offset of the lane's r slice
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    gb_off[i] = comp_of[i] * G3H;
    gbi_off[i] = (uint32_t)(comp_of[i] * G3H + c_col * 8) * (uint32_t)sizeof(T);
  }
  if constexpr (GB_REGS) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const T* grow = gamma + gb_off[i];
      const T* brow = beta + gb_off[i];
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
          int col = g * H + nt * 16 + c_col;
          uint16_t gv = live[i] ? f2bf(ldf(grow + col)) : 0;
          uint16_t bv = live[i] ? f2bf(ldf(brow + col)) : 0;
          gb[i][g][nt] = ((uint32_t)bv << 16) | gv;
        }
    }
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) bh[g][nt] = b_hh[g * H + nt * 16 + c_col];
  }

  // ---- fp32 hidden state in registers + bf16 tile in LDS ----
  float h[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
      int col = nt * 16 + c_col;
      float v = live[i] ? ldf(h0 + ((int64_t)b_of[i] * C + comp_of[i]) * H + col) : 0.f;
      h[i][nt] = v;
      if constexpr (FP8)
        *reinterpret_cast<uint8_t*>(Hl + swz8(row_of[i], col)) = f2fp8(v);
      else
        *reinterpret_cast<uint16_t*>(Hl + swz(row_of[i], col)) = f2bf(v);
    }

  // ---- t-invariant descriptors ----
  // The expensive per-step address math was the runtime divisions (r / C)
  // and 64-bit muls: precompute ROW indices once, share ONE per-step time
  // offset, and derive addresses with shifts/adds.
  const int t_first = reverse ? (TT - 1) : 0;
  const int dirC = (reverse ? -1 : 1) * C;           // row-index per-t stride

  // xg staging, per wave: wave wv stages only the batches its own 16 rows
  // span, into its own WSLOTS slots of the XG region, so the time loop needs
  // no workgroup barrier.  16 consecutive rows span at most ceil(15/C)+1
  // batches: 6 at C >= 3 (4 waves x 6 slots), 4 at C >= 5, the 8-wave
  // variant's dispatch condition (8 waves x 4 slots).  The chunks (slot, blk
  // fixed over t) are dealt over the wave's 64 lanes; offsets are 32-bit
  // (binding checks xg.numel() < 2^31).
  constexpr int WSLOTS = NSUB == 2 ? 4 : 6;
  static_assert(WAVES * NSUB * WSLOTS <= XG_SLOTS,
                "per-wave xg slots exceed the XG region");
  constexpr int MAXCH = (WSLOTS * (G3H / 8) + DR_WAVE - 1) / DR_WAVE;  // 3 or 5
  const int b_wlo = (int)(std::min<int64_t>(r0 + wv * 16, R - 1) / C);
  int stage_soff[MAXCH];    // xg element offset at t_first
  int stage_pi0[MAXCH];     // pi-layout LDS element offset of the chunk
  int n_stage = 0;
  {
    int n_b = (int)(std::min<int64_t>(r0 + wv * 16 + 15, R - 1) / C) - b_wlo + 1;
    n_b = std::min(n_b, WSLOTS);   // never binds under the dispatch conditions;
                                   // keeps every LDS index inside the wave's slots
    for (int id = lane; id < n_b * (G3H / 8) && n_stage < MAXCH; id += DR_WAVE) {
      int slot = id / (G3H / 8);
      int blk = id % (G3H / 8);
      int j0 = blk * 8;
      int g = j0 >> 7;
      int col0 = j0 & 127;
      stage_soff[n_stage] = (int)((((int64_t)(b_wlo + slot) * TT) + t_first) * G3H) + j0;
      stage_pi0[n_stage] =
          (wv * WSLOTS + slot) * G3H + g * H + ((col0 & 15) << 3) + (col0 >> 4);
      ++n_stage;
    }
  }
  // ONE 32-bit row index per lane row, (b*TT + t_first)*C + c, shared by the
  // saves, h_all and out stores and widened at the multiply (the binding
  // checks B*TT*C < 2^31 and, with heads, B*TT*C*O < 2^31)
  int bc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    bc[i] = (b_of[i] * TT + t_first) * C + comp_of[i];
  // per-wave A-fragment LDS offsets
  int afrag_off[KT];
  {
    int arow = wv * 16 + (lane & 15);
    int k0 = (lane >> 4) * 8;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
      afrag_off[kt] = FP8 ? swz8(arow, kt * 32 + k0) : swz(arow, kt * 32 + k0);
  }
  // xg LDS row bases in the wave's own slots (pi layout, element-indexed).
  // Keep the operand order: with c_col * 8 added first the spilling FP8 tile
  // came out at 176 B of scratch instead of 76 / 92.
  const uint16_t* xg_rows[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    xg_rows[i] =
        reinterpret_cast<const uint16_t*>(XGl) +
        (wv * WSLOTS + std::min(b_of[i] - b_wlo, WSLOTS - 1)) * G3H + c_col * 8;

  __syncthreads();   // W / wh_fwd staging visible to all waves

  // ---- time loop: no workgroup barrier inside ----
  // Everything a wave reads from the h mirror and the XG region it wrote
  // itself: its A-fragments, head fragments and h_all chunks are its own 16
  // mirror rows, its xg_rows its own slots.  A wave's LDS operations execute
  // in issue order, so its own write-then-read needs no s_barrier; the
  // wavefront-scope fences below only keep the compiler from moving those
  // accesses across each other.  Waves free-run: one wave's MFMA / LDS phase
  // overlaps the other wave's epilogue on the same SIMD.
  int stage_toff = 0;                        // += dir*G3H per step (32-bit)
  int bc_toff = 0;                           // += dirC per step (row-index units)
  const int stage_tstep = (reverse ? -1 : 1) * G3H;
  for (int step = 0; step < TT; ++step) {
    // VARLEN: row i is active at this step iff t_now < len_of[i]
    const int t_now = reverse ? (TT - 1 - step) : step;
    (void)t_now;
    // opaque per step: keeps the streamed operand loads inside the loop
    uint32_t zoff = 0;
    if constexpr (!GB_REGS) zoff = opaque_zero();
    (void)zoff;
    // A-fragments: this wave's 16 rows of the h tile, all 4 K-tiles
    bf16x8 afrag[KT];
    int64_t afrag8[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      if constexpr (FP8)
        afrag8[kt] = *reinterpret_cast<const int64_t*>(Hl + afrag_off[kt]);
      else
        afrag[kt] = lds_read8(Hl, afrag_off[kt]);
    }

    // stage xg[., t, :] into LDS in pi layout: the 8 loaded naturals land at
    // positions pi_0 + 8e (16 B stride), so a (row, gate) slice is 16
    // contiguous bytes: ONE ds_read_b128 in the streaming epilogue (the
    // register-holding tiles still read it as 8 ds_read_u16, see there).
#pragma unroll
    for (int u = 0; u < MAXCH; ++u) {        // compile-time index (rule 20)
      if (u < n_stage) {
        const T* src = xg + stage_soff[u] + stage_toff;
        uint16_t* dst = reinterpret_cast<uint16_t*>(XGl) + stage_pi0[u];
        uint16_t vals[8];
        ld_raw8(src, vals);
#pragma unroll
        for (int e = 0; e < 8; ++e) dst[e * 8] = vals[e];
      }
    }
    // the slot writes above stay ahead of this step's epilogue reads (other
    // lanes of this wave read them), and this step's mirror writes behind the
    // previous step's h_all / head reads
    wave_lds_fence();

    // ---- MFMA: hh = h_tile @ W^T -> (64, 384), this wave's 16 rows ----
    // One tile at a time, each MFMA behind its own fragment read.  Advancing
    // several tiles together with the reads ahead of the MFMAs (groups of 2
    // and 4, with and without a double buffer) put every HEADS variant of the
    // 8-wave tile 4 to 12 registers into scratch; see
    // profiles/r12_gru_epilogue.md.
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        int j = nt * 16 + c_col;                       // W row (gate col)
        int k0 = kt * 32 + (lane >> 4) * 8;
        if constexpr (FP8) {
          int64_t bfrag = *reinterpret_cast<const int64_t*>(Wl + swz8(j, k0));
          a = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(afrag8[kt], bfrag, a, 0, 0, 0);
        } else {
          bf16x8 bfrag = lds_read8(Wl, swz(j, k0));
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[kt], bfrag, a, 0, 0, 0);
        }
      }
      acc[nt] = a;
    }

    // ---- fused gate epilogue (vectorized pi-layout saves) ----
    if constexpr (GB_REGS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float fr[8], fz[8];
        bool active = true;
        if constexpr (VARLEN) active = t_now < len_of[i];
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
          // pi layout: the 8 values of a gate are 16 consecutive LDS bytes.
          // Read one by one here (8 ds_read_u16 per gate): the 16-byte read
          // of the streaming branch put these register-holding tiles into
          // scratch.
          float xr = bf2f(xg_rows[i][nt]);
          float xz = bf2f(xg_rows[i][H + nt]);
          float xn = bf2f(xg_rows[i][2 * H + nt]);
          int col = nt * 16 + c_col;
          float gmr = bf2f((uint16_t)gb[i][0][nt]), btr = bf2f((uint16_t)(gb[i][0][nt] >> 16));
          float gmz = bf2f((uint16_t)gb[i][1][nt]), btz = bf2f((uint16_t)(gb[i][1][nt] >> 16));
          float gmn = bf2f((uint16_t)gb[i][2][nt]), btn = bf2f((uint16_t)(gb[i][2][nt] >> 16));
          float bhr = bh[0][nt], bhz = bh[1][nt], bhn = bh[2][nt];
          float g_r = xr * gmr + btr;
          float g_z = xz * gmz + btz;
          float g_n = xn * gmn + btn;
          float rp = sigmoidf_(acc[nt][i] + bhr + g_r);
          float zp = sigmoidf_(acc[nt + 8][i] + bhz + g_z);
          float hn = acc[nt + 16][i] + bhn;
          float nn = tanhf_(g_n + rp * hn);
          float hnew = (1.f - zp) * nn + zp * h[i][nt];
          if constexpr (VARLEN) hnew = active ? hnew : h[i][nt];
          h[i][nt] = hnew;
          if constexpr (FP8)
            *reinterpret_cast<uint8_t*>(Hl + swz8(row_of[i], col)) = f2fp8(hnew);
          else
            *reinterpret_cast<uint16_t*>(Hl + swz(row_of[i], col)) = f2bf(hnew);
          fr[nt] = rp; fz[nt] = zp;
        }
        if (SAVE && live[i]) {
          // only r and z are saved (2H); the backward recomputes n and hh_n
          // (an extra H x H GEMM there is cheaper than 2H of HBM both ways)
          T* sv = saves + (int64_t)(bc[i] + bc_toff) * (2 * H) + c_col * 8;
          st8(sv, fr);
          st8(sv + H, fz);
        }
        // fence: stop the scheduler interleaving all 4 rows' live ranges
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      // Streaming variants.  The epilogue is 12 stages, (row, gate) in the
      // order r, z, n.  A stage's operands are three 16-byte reads: gamma and
      // beta from the pi images (global, f32: two each) and x_gates from the
      // wave's pi-ordered slot (one ds_read_b128).  The global ones are
      // issued one stage AHEAD (bf16 IO), so their latency passes under the
      // previous stage's eight sigmoids / tanhs; the LDS read stays at the
      // head of its own stage (4 more registers in flight spill).  The
      // scheduling barriers keep that order and keep the stages' live ranges
      // apart.
      struct Stage { Raw8<T> gm, bt; };
      auto issue = [&](int i, int g) {
        const uint32_t off = gbi_off[i] + zoff + (uint32_t)(g * H * sizeof(T));
        return Stage{ld_raw_at<T>(gamma, off), ld_raw_at<T>(beta, off)};
      };
      // gate pre-activation x * gamma + beta of one stage, 8 N-tiles
      auto film = [&](const Stage& st, int i, int g, float* out) {
        float xv[8], gmv[8], btv[8];
        widen8(Raw8<uint16_t>{*reinterpret_cast<const uint4*>(xg_rows[i] + g * H)}, xv);
        widen8(st.gm, gmv);
        widen8(st.bt, btv);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
          if constexpr (NSUB == 1) {
            // Streamed twin of the packed registers (the lengths FP8 tile):
            // the same bf16-rounded values, and what -ffp-contract leaves to
            // the compiler pinned to what the register-held kernel does —
            // there the r and z products are rounded before beta is added
            // and only the n gate is contracted into an FMA.
            float gm = gmv[nt], bt = btv[nt];
            if constexpr (sizeof(T) == 4) { gm = bf2f(f2bf(gm)); bt = bf2f(f2bf(bt)); }
            out[nt] = g < 2 ? mul_rounded(xv[nt], gm) + bt : __builtin_fmaf(xv[nt], gm, bt);
          } else {
            // the 8-wave tile contracts all three into FMAs, as it always has
            out[nt] = __builtin_fmaf(xv[nt], gmv[nt], btv[nt]);
          }
        }
      };
      // b_hh joins the accumulators once per step: six 16-byte loads serve
      // all four rows
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        float bv[8];
        widen8(ld_raw_at<float>(b_hh, (uint32_t)(g * H + c_col * 8) * 4u + zoff), bv);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[g * 8 + nt][i] += bv[nt];
      }
      // Mirror write addresses, all 32 from ONE register: row i of the lane
      // and N-tile nt only flip bits of the swizzled block index of (row 0,
      // tile 0) — one XOR with a constant — and the row's byte offset goes
      // into the instruction's offset field.  Opaque per step, or the 32
      // addresses come back as loop-invariant registers.
      constexpr int MIRROR_ROW_SHIFT = FP8 ? 3 : 4;    // 8 / 16 B blocks
      constexpr int MIRROR_NT_SHIFT = MIRROR_ROW_SHIFT + 1;
      constexpr int MIRROR_ROW_BYTES = FP8 ? 128 : 256;
      const int hm0 = (FP8 ? swz8(row_of[0], c_col) : swz(row_of[0], c_col)) + (int)zoff;
      // f32 IO: a stage is 20 registers, and a second one in flight spills;
      // those tiles issue each stage's loads at its own head.
      constexpr bool AHEAD = sizeof(T) == 2;
      Stage cur, nxt;
      if constexpr (AHEAD) cur = issue(0, 0);
      __builtin_amdgcn_sched_barrier(0);
      float fr[8], fz[8];
#pragma unroll
      for (int s = 0; s < 12; ++s) {
        const int i = s / 3, g = s % 3;
        if constexpr (AHEAD) {
          if (s + 1 < 12) nxt = issue((s + 1) / 3, (s + 1) % 3);
        } else {
          cur = issue(i, g);
        }
        float pre[8];
        film(cur, i, g, pre);
        if (g == 0) {
#pragma unroll
          for (int nt = 0; nt < 8; ++nt) fr[nt] = sigmoidf_(acc[nt][i] + pre[nt]);
        } else if (g == 1) {
#pragma unroll
          for (int nt = 0; nt < 8; ++nt) fz[nt] = sigmoidf_(acc[nt + 8][i] + pre[nt]);
        } else {
          bool active = true;
          if constexpr (VARLEN) active = t_now < len_of[i];
#pragma unroll
          for (int nt = 0; nt < 8; ++nt) {
            const float hn = acc[nt + 16][i];
            const float rp = fr[nt], zp = fz[nt];
            float nn = tanhf_(pre[nt] + rp * hn);
            // the blend, pinned like the gate sums above: the 8-wave tile
            // contracts z * h into the sum, the register-held kernels (and
            // so their streamed twin) round both products first
            float hnew;
            if constexpr (NSUB == 1)
              hnew = mul_rounded(1.f - zp, nn) + mul_rounded(zp, h[i][nt]);
            else
              hnew = __builtin_fmaf(zp, h[i][nt], mul_rounded(1.f - zp, nn));
            if constexpr (VARLEN) hnew = active ? hnew : h[i][nt];
            h[i][nt] = hnew;
            // XOR, not OR: row bit 1 and N-tile bit 0 meet in the same bit
            char* hm_p = Hl + (hm0 ^ ((i << MIRROR_ROW_SHIFT) ^ (nt << MIRROR_NT_SHIFT))) +
                         i * MIRROR_ROW_BYTES;
            if constexpr (FP8)
              *reinterpret_cast<uint8_t*>(hm_p) = f2fp8(hnew);
            else
              *reinterpret_cast<uint16_t*>(hm_p) = f2bf(hnew);
          }
          if (SAVE && live[i]) {
            // only r and z are saved (2H); the backward recomputes n and hh_n
            // (an extra H x H GEMM there is cheaper than 2H of HBM both ways)
            T* sv = saves + (int64_t)(bc[i] + bc_toff) * (2 * H) + c_col * 8;
            st8(sv, fr);
            st8(sv + H, fz);
          }
        }
        if constexpr (AHEAD) cur = nxt;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // the mirror rows written above are read below and at the top of the next
    // step by other lanes of this wave; the next step's slot writes stay
    // behind the xg reads above
    wave_lds_fence();

    if constexpr (HEADS) {
      // ---- head phase: out[rows, t, :O] = h_t @ w_head^T ----
      // A-fragments: this wave's own 16 rows of the just-written h mirror
      // (the reads that open the next step).  FP8: the e4m3 mirror values
      // are bf16-representable, so the conversion is exact and the heads see
      // what the h_all store of the plain kernel would have written.
      bf16x8 hfrag[KT];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        if constexpr (FP8) {
          uint64_t raw = *reinterpret_cast<const uint64_t*>(Hl + afrag_off[kt]);
          const uint8_t* q = reinterpret_cast<const uint8_t*>(&raw);
          uint16_t p[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            __hip_fp8_e4m3 x;
            x.__x = q[e];
            p[e] = f2bf(float(x));
          }
          hfrag[kt] = *reinterpret_cast<const bf16x8*>(p);
        } else {
          hfrag[kt] = lds_read8(Hl, afrag_off[kt]);
        }
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        if (nt * 16 < O) {                     // wave-uniform
          f32x4 a = {0.f, 0.f, 0.f, 0.f};
          const int j = nt * 16 + c_col;       // head output column
#pragma unroll
          for (int kt = 0; kt < KT; ++kt) {
            const int k0 = kt * 32 + (lane >> 4) * 8;
            bf16x8 bfrag = lds_read8(WHl, swz(j, k0));
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hfrag[kt], bfrag, a, 0, 0, 0);
          }
          if (j < O) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (live[i] && (!VARLEN || t_now < len_of[i]))
                stf(out + (bc[i] + bc_toff) * O + j, a[i]);
          }
        }
      }
    }
    if constexpr (!HEADS || SAVE) {
      // ---- h_all store: lane (rgrp, c_col) stores chunk c_col (8 values) of
      // its own 4 rows from the mirror; 16 lanes cover one row ----
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (live[u]) {
          T* dst = h_all + (int64_t)(bc[u] + bc_toff) * H + c_col * 8;
          const int row = row_of[u];
          if constexpr (FP8) {
            uint64_t raw = *reinterpret_cast<const uint64_t*>(
                Hl + row * 128 + ((c_col ^ (row & 15)) << 3));
            const uint8_t* q = reinterpret_cast<const uint8_t*>(&raw);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              __hip_fp8_e4m3 x;
              x.__x = q[e];
              stf(dst + e, float(x));
            }
          } else {
            st_frag(dst, lds_read8(Hl, row * 256 + ((c_col ^ (row & 15)) << 4)));
          }
        }
      }
    }
    stage_toff += stage_tstep;
    bc_toff += dirC;
    // no end-of-step barrier: the next epilogue's mirror writes follow the
    // reads above in this wave's own issue order (fence at the next staging)
  }

  if constexpr (HEADS && !SAVE) {
    // ---- h_last: the fp32 register state, rounded once to the IO dtype ----
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!live[i]) continue;
      T* dst = h_last + r_abs[i] * H + c_col;   // row b*C + c is r_abs itself
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) stf(dst + nt * 16, h[i][nt]);
    }
  }
}

// ---------------------------------------------------------------- backward
// The MFMA K axis runs over pi positions m in [0, 384): regions {dr, dz,
// d_hhn}, the first three slices of a dpre row (dn, which only feeds the
// x-side, comes last).  A-fragments read the just-written GLOBAL dpre rows (same-CU L2
// after __syncthreads); the B image in LDS is W^T with rows permuted to the
// same m ordering, so both sides agree on any K permutation.
// NSUB = 1: 4 waves / 64 rows, no LDS, W streamed from L2 (2 blocks/CU can
//           co-reside when the grid exceeds the CU count).
// NSUB = 2: 8 waves / 128 rows, the pi-permuted W image staged ONCE in LDS
//           (96 KB) — 2 waves/SIMD from one block with low-latency
//           B-fragments; used when the grid still fills the chip.
// FUSED: the upstream gradient arrives as the quantile heads' narrow output
//        gradient grad_part (B, TT, C, O), O <= 32, instead of grad_h.  Per
//        step one K=32 MFMA per 16-column tile forms grad_part @ w_head
//        straight into the dh_carry accumulators (same C-fragment layout),
//        so the (B, TT, C, H) head input gradient is never materialized.
template <typename T, int NSUB, bool FUSED>
__global__ __launch_bounds__(NSUB * THREADS) void gru_bwd_kernel(
    const T* __restrict__ grad_h,   // (B, TT, C, H); FUSED: grad_part (B, TT, C, O)
    const uint16_t* __restrict__ wh_img,  // FUSED: (H, 32) bf16, wh_img[n][k] =
                                          // w_head[k][n], zero for k >= O
    const uint16_t* __restrict__ w_img,  // (H, 384) bf16: w_img[k][m] = W[natJ(m)][k]
    const uint16_t* __restrict__ w_fwd,  // (3H, H) bf16 natural layout
    const T* __restrict__ xg,       // (B, TT, 3H)
    const T* __restrict__ gamma,    // (C, 3H) pi-ordered operand image
    const T* __restrict__ beta,     // (C, 3H) pi-ordered operand image
    const float* __restrict__ b_hh, // (3H,) natural order
    const T* __restrict__ h0,       // (B, C, H)
    const T* __restrict__ h_all,    // (B, TT, C, H)
    const T* __restrict__ saves,    // (B, TT, C, 2H) pi layout: r|z
    T* __restrict__ dpre,           // (B, TT, C, 4H) pi: dr|dz|d_hhn|dn
    float* __restrict__ dh0,        // (B, C, H)
    int B, int TT, int C, int reverse, int O) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using L = BwdLds<NSUB, FUSED>;       // the pi W image sits at smem itself
  char* wn_lds = smem + L::WN;         // (NSUB==2) W_hn rows
  char* wh_lds = smem + L::WH;         // (NSUB==2, FUSED) head weight image
  const int tid = threadIdx.x;
  const int wv = tid / DR_WAVE;
  const int lane = tid % DR_WAVE;
  const int64_t R = (int64_t)B * C;
  const int64_t r0 = (int64_t)blockIdx.x * (ROWS * NSUB);

  if constexpr (NSUB == 2) {
    // stage the pi W image (dh GEMM), swz768-swizzled rows [k_h][m]
    for (int id = tid; id < H * (G3H / 8); id += NSUB * THREADS) {
      int k = id / (G3H / 8);
      int mblk = id % (G3H / 8);
      bf16x8 v = *reinterpret_cast<const bf16x8*>(w_img + (int64_t)k * G3H + mblk * 8);
      *reinterpret_cast<bf16x8*>(smem + k * 768 + ((mblk ^ (k & 15)) << 4)) = v;
    }
    // stage W_hn rows (hh_n recompute GEMM), fwd-style [j][k] swizzled
    for (int id = tid; id < H * (H / 8); id += NSUB * THREADS) {
      int jl = id / (H / 8);
      int blk = id % (H / 8);
      bf16x8 v = *reinterpret_cast<const bf16x8*>(
          w_fwd + (int64_t)(2 * H + jl) * H + blk * 8);
      *reinterpret_cast<bf16x8*>(wn_lds + jl * 256 + ((blk ^ (jl & 15)) << 4)) = v;
    }
    // head weight image (8 KB), linear [n][32]: a wave's 64 fragment reads
    // per N-tile cover 1 KB contiguous, so no swizzle is needed
    if constexpr (FUSED) {
      for (int id = tid; id < H * 4; id += NSUB * THREADS)
        *reinterpret_cast<bf16x8*>(wh_lds + id * 16) =
            *reinterpret_cast<const bf16x8*>(wh_img + id * 8);
    }
  }

  const int c_col = lane & 15;
  const int rgrp = lane >> 4;
  int row_of[4];
  int64_t r_abs[4];
  int b_of[4], comp_of[4];
  bool live[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    row_of[i] = wv * 16 + rgrp * 4 + i;
    r_abs[i] = r0 + row_of[i];
    live[i] = r_abs[i] < R;
    int64_t rr = live[i] ? r_abs[i] : (R - 1);
    b_of[i] = (int)(rr / C);
    comp_of[i] = (int)(rr % C);
  }

  // dh carry in MFMA C-fragment order: dh_carry[nt][i] <-> (row rgrp*4+i,
  // col nt*16+c_col).  Kept as scalars (an f32x4 array pinned the unfused
  // variants to register quads: +11 VGPRs, scratch on the fp32 one); the
  // FUSED head MFMA gathers/scatters one tile's four values around itself.
  float dh_carry[8][4];
#pragma unroll
  for (int nt = 0; nt < 8; ++nt)
#pragma unroll
    for (int i = 0; i < 4; ++i) dh_carry[nt][i] = 0.f;
  if constexpr (NSUB == 2) __syncthreads();  // W staging visible to all waves

  // ---- compact addressing: per-row indices + ONE shared per-step offset ----
  // (pointer arrays spilled; full recompute burned VALU on divisions — this
  // derives every address from bc[i] + bc_toff with shifts/adds)
  const int t_first = reverse ? 0 : (TT - 1);
  const int dirC = (reverse ? 1 : -1) * C;
  int64_t bc0[4];           // (b*TT + t_first)*C + c per owned row
  int64_t h0_off[4];        // h0 row offset (t-invariant)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bc0[i] = ((int64_t)b_of[i] * TT + t_first) * C + comp_of[i];
    h0_off[i] = ((int64_t)b_of[i] * C + comp_of[i]) * H;
  }
  const int arow = wv * 16 + (lane & 15);
  const int64_t ra = (r0 + arow < R) ? (r0 + arow) : (R - 1);
  const int ab = (int)(ra / C), ac = (int)(ra % C);
  const int64_t abc0 = ((int64_t)ab * TT + t_first) * C + ac;
  const int64_t h0_off_a = ((int64_t)ab * C + ac) * H;
  const int k0 = (lane >> 4) * 8;
  // per-row xg bases + t-invariant b_hh n-slice
  int64_t xgb0[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    xgb0[i] = ((int64_t)b_of[i] * TT + t_first) * G3H;
  float bhn[8];
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) bhn[nt] = b_hh[2 * H + nt * 16 + c_col];

  int64_t bc_toff = 0;      // += dirC per step
  int64_t xg_toff = 0;      // += dir*G3H per step
  const int64_t xg_step = (reverse ? 1 : -1) * (int64_t)G3H;
  for (int step = 0; step < TT; ++step) {
    // the FIRST processed step is the forward pass's LAST, whose h_prev is
    // h_all of the step before; h0 is the prev only at the LAST processed
    // step (= forward t boundary)
    const bool use_h0 = (step == TT - 1);

    if constexpr (FUSED) {
      // ---- dh_carry += grad_part[rows, :O] @ w_head (one K=32 MFMA/tile) ----
      // A-fragment: lane (arow, k0) holds grad_part[arow, k0..k0+7].  The
      // address is clamped into the row and k >= O is forced to exact zero
      // (select, not a branch: every lane issues the same 8 loads).
      const T* gp = grad_h + (abc0 + bc_toff) * O;
      uint16_t av[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = k0 + j;
        const T raw = gp[k < O ? k : O - 1];
        uint16_t b;
        if constexpr (sizeof(T) == 2) b = (uint16_t)raw; else b = f2bf(raw);
        av[j] = (k < O) ? b : (uint16_t)0;
      }
      const bf16x8 afrag = *reinterpret_cast<const bf16x8*>(av);
      const uint16_t* whv = wh_img;
      if constexpr (NSUB == 1) asm volatile("" : "+v"(whv));
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        const int n = nt * 16 + c_col;
        bf16x8 bfrag;
        if constexpr (NSUB == 2)
          bfrag = lds_read8(wh_lds, n * 64 + k0 * 2);
        else
          bfrag = *reinterpret_cast<const bf16x8*>(whv + n * 32 + k0);
        f32x4 c = {dh_carry[nt][0], dh_carry[nt][1], dh_carry[nt][2],
                   dh_carry[nt][3]};
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag, bfrag, c, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) dh_carry[nt][i] = c[i];
      }
    }

    // ---- recompute hh_n = h_prev @ W_hn^T for this wave's 16 rows ----
    // (saving it cost 2H of HBM each way; one extra HxH MFMA pass is cheaper)
    f32x4 hhn_acc[8];
    {
      const uint16_t* wfv = w_fwd;
      if constexpr (NSUB == 1) asm volatile("" : "+v"(wfv));
      const T* hsrc_a = use_h0 ? (h0 + h0_off_a)
                               : (h_all + (abc0 + bc_toff + dirC) * H);
      bf16x8 hfrag[KT];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
        hfrag[kt] = ld_frag(hsrc_a + kt * 32 + k0);
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        const int jl = nt * 16 + c_col;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          bf16x8 bfrag;
          if constexpr (NSUB == 2)
            bfrag = lds_read8(wn_lds, swz(jl, kt * 32 + k0));
          else
            bfrag = *reinterpret_cast<const bf16x8*>(
                wfv + (int64_t)(2 * H + jl) * H + kt * 32 + k0);
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hfrag[kt], bfrag, a, 0, 0, 0);
        }
        hhn_acc[nt] = a;
      }
    }

    const uint32_t zoff = opaque_zero();   // keeps the FiLM loads in the loop
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!live[i]) continue;
      const int64_t bc = bc0[i] + bc_toff;
      const T* sv_p = saves + bc * (2 * H) + c_col * 8;
      float rp[8], zp[8];
      ld8(sv_p, rp);
      ld8(sv_p + H, zp);
      float fdr[8], fdz[8], fdn[8], fdh[8];
      // h_prev sits at bc + dirC rows (tprev = t+dir); h0 at the boundary.
      // pointer select -> ONE load (the OOB address is never dereferenced)
      const T* hsrc = use_h0 ? (h0 + h0_off[i])
                             : (h_all + (bc + dirC) * H);
      const T* gr_p = grad_h + bc * H;   // !FUSED only
      const T* xg_n = xg + xgb0[i] + xg_toff + 2 * H;
      // the n slices of the row's FiLM operands: one 16-byte load each
      // from the pi images (f32: two)
      float gmn[8], btn[8];
      {
        const uint32_t off =
            (uint32_t)(comp_of[i] * G3H + 2 * H + c_col * 8) * (uint32_t)sizeof(T) + zoff;
        const Raw8<T> gq = ld_raw_at<T>(gamma, off);
        const Raw8<T> bq = ld_raw_at<T>(beta, off);
        widen8(gq, gmn);
        widen8(bq, btn);
      }
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        int col = nt * 16 + c_col;
        float hp = ldf(hsrc + col);
        // recompute the n gate: hh_n from the GEMM above, g_n from xg/FiLM
        float hn = hhn_acc[nt][i] + bhn[nt];
        float g_n = ldf(xg_n + col) * gmn[nt] + btn[nt];
        float nn = tanhf_(g_n + rp[nt] * hn);
        float dht = dh_carry[nt][i];       // FUSED: head term already in
        if constexpr (!FUSED) dht += ldf(gr_p + col);
        float dz = dht * (hp - nn);
        float dn = dht * (1.f - zp[nt]);
        float dnp = dn * (1.f - nn * nn);
        float dhhn = dnp * rp[nt];
        float dr = dnp * hn;
        fdr[nt] = dr * rp[nt] * (1.f - rp[nt]);
        fdz[nt] = dz * zp[nt] * (1.f - zp[nt]);
        fdn[nt] = dnp;
        fdh[nt] = dhhn;
        dh_carry[nt][i] = dht * zp[nt];    // partial; MFMA adds dpre @ W
      }
      T* dx_p = dpre + bc * G4H + c_col * 8;
      st8(dx_p, fdr);
      st8(dx_p + H, fdz);
      st8(dx_p + 2 * H, fdh);
      st8(dx_p + 3 * H, fdn);
      // fence the scheduler: without this it interleaves all 4 row
      // iterations and the combined live ranges spill to scratch
      __builtin_amdgcn_sched_barrier(0);
    }
    // Every A-fragment row this wave reads was written by THIS wave's own
    // lanes (rows wv*16..wv*16+15), so no cross-wave barrier is needed —
    // only completion of our own stores (same-CU L1/L2 then serves the
    // cross-lane reads).  Waves free-run, which is worth real latency
    // hiding on this memory-bound kernel.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- MFMA: delta = dpre_pi (64 x 384 over m) @ W_pi, wave's 16 rows ----
    {
      // NSUB==1: opaque copy of the W pointer stops LLVM from hoisting all
      // 96 loop-invariant B-fragment loads out of the t loop (384 registers
      // -> scratch); W streams from L1/L2 each step by design.
      const uint16_t* w_imgv = w_img;
      if constexpr (NSUB == 1) asm volatile("" : "+v"(w_imgv));
      const T* arow_p = dpre + (abc0 + bc_toff) * G4H;
      bf16x8 afrag[12];
#pragma unroll
      for (int kt = 0; kt < 12; ++kt)
        afrag[kt] = ld_frag(arow_p + kt * 32 + k0);
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        const int n = nt * 16 + c_col;
        const uint16_t* wrow = w_imgv + (int64_t)n * G3H;
#pragma unroll
        for (int kt = 0; kt < 12; ++kt) {
          bf16x8 bfrag;
          if constexpr (NSUB == 2)
            bfrag = lds_read8(smem, swz768(n, kt * 32 + k0));
          else
            bfrag = *reinterpret_cast<const bf16x8*>(wrow + kt * 32 + k0);
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[kt], bfrag, a, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) dh_carry[nt][i] += a[i];
      }
    }
    bc_toff += dirC;
    xg_toff += xg_step;
    // no end-of-step barrier: the next step's stores go to DIFFERENT dpre
    // addresses (per-t storage); the W images are read-only.
  }

  // ---- dh0 = final carry ----
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) {
    int col = nt * 16 + c_col;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!live[i]) continue;
      dh0[((int64_t)b_of[i] * C + comp_of[i]) * H + col] = dh_carry[nt][i];
    }
  }
}

// ------------------------------------------------- backward reductions
// One pass over dpre per kernel (replaces the einsum broadcasts that
// dominated the profiled step).  All kernels understand the pi layout and
// dpre's slice order dr|dz|d_hhn|dn, and emit NATURAL-order outputs.  The
// x-side gates (r, z, n) are slices 0, 1, 3; slice 2 (d_hhn) only feeds
// dbeta4, whose slices follow dpre's order.
//   C <= REDUCE_FUSED_MAX_C: gru_reduce_fused_kernel reads each row once.
//   above (or on request):   gru_dxg_kernel + gru_dgamma_kernel, two reads.

// dpre slice of x-side gate g, and the gate a slice feeds (-1: none)
__device__ __forceinline__ int slice_of_gate(int g) { return g < 2 ? g : 3; }
__device__ __forceinline__ int gate_of_slice(int s) {
  return s < 2 ? s : (s == 3 ? 2 : -1);
}

// natural (r, 3H) -> pi-layout copy: position g*H + cc*8 + e holds natural
// column g*H + cc + 16e.  Run ONCE per tensor so the reduction kernels'
// inner loops replace 8 scalar loads with one 16-byte vector load (the
// scalar-load issue rate, not HBM bandwidth, bounded the old versions).
template <typename T>
__global__ void pi_permute_rows_kernel(const T* __restrict__ in,
                                       T* __restrict__ out, int64_t N) {
  const int64_t n_chunks = N * 48;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < n_chunks; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = idx / 48;
    const int rem = (int)(idx % 48);
    const int g = rem / 16;
    const int cc = rem % 16;
    const T* src = in + r * G3H + g * H + cc;
    T* dst = out + r * G3H + g * H + cc * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[e] = src[e * 16];
  }
}

// Pi-ordered images of the t-invariant operands the streaming chain kernels
// re-read every step: gamma and beta (C, 3H) in the IO dtype, b_hh (3H) in
// f32, in ONE buffer [gamma_pi | beta_pi | bhh_pi] that the caller allocates
// (operand_images_bytes) and one launch fills.  The values are copied, not
// converted.  Built per call: the tensors are parameters that change between
// steps, and the copy is 2C + 1 rows.
template <typename T>
struct OperandImages {
  static int64_t gamma(int C) { (void)C; return 0; }
  static int64_t beta(int C) { return (int64_t)C * G3H * (int64_t)sizeof(T); }
  static int64_t bhh(int C) { return 2 * beta(C); }
  static int64_t total(int C) { return bhh(C) + G3H * 4; }
};

template <typename T>
__global__ void gru_operand_images_kernel(const T* __restrict__ gamma,
                                          const T* __restrict__ beta,
                                          const float* __restrict__ b_hh,
                                          T* __restrict__ gamma_pi,
                                          T* __restrict__ beta_pi,
                                          float* __restrict__ bhh_pi, int C) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (2 * C + 1) * 48) return;
  const int r = idx / 48;
  const int rem = idx % 48;
  const int src = (rem / 16) * H + rem % 16;        // natural column of element 0
  const int dst = (rem / 16) * H + (rem % 16) * 8;  // its pi position
  if (r < 2 * C) {
    const T* in = (r < C ? gamma + r * G3H : beta + (r - C) * G3H) + src;
    T* out = (r < C ? gamma_pi + r * G3H : beta_pi + (r - C) * G3H) + dst;
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = in[e * 16];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) bhh_pi[dst + e] = b_hh[src + e * 16];
  }
}

// dxg[bt, j] = sum_c dpre[bt, c, pi(j)] * gamma[c, j]   (j in [0, 3H))
// thread chunk = (bt, gate, c_col): 8 pi-contiguous dpre values per c.
// gamma_pi is the pi-permuted gamma image: one ld8 per c instead of 8
// scalar loads (tiny tensor, L1/L2-resident across all bt chunks).
template <typename T>
__global__ void gru_dxg_kernel(const T* __restrict__ dpre,     // (BT, C, 4H) pi
                               const T* __restrict__ gamma_pi, // (C, 3H) pi
                               T* __restrict__ dxg,            // (BT, 3H)
                               int64_t BT, int C) {
  const int64_t n_chunks = BT * 48;      // 3 gates x 16 c_col groups
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n_chunks;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t bt = idx / 48;
    const int rem = (int)(idx % 48);
    const int g = rem / 16;
    const int cc = rem % 16;
    const int pi0 = g * H + cc * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    const T* base = dpre + bt * C * G4H + slice_of_gate(g) * H + cc * 8;
    // 4x unroll: the c loop has a runtime bound, so without it the
    // compiler keeps ONE 1-KB wave read in flight and the kernel is
    // latency-bound at ~2.7 TB/s (measured; 4 concurrent reads ~ 4x MLP)
    int c = 0;
    for (; c + 4 <= C; c += 4) {
      float d[4][8], gm[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        ld8(base + (int64_t)(c + u) * G4H, d[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        ld8(gamma_pi + (int64_t)(c + u) * G3H + pi0, gm[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += d[u][e] * gm[u][e];
    }
    for (; c < C; ++c) {
      float d[8], gm[8];
      ld8(base + (int64_t)c * G4H, d);
      ld8(gamma_pi + (int64_t)c * G3H + pi0, gm);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += d[e] * gm[e];
    }
    T* out = dxg + bt * G3H + g * H + cc;
#pragma unroll
    for (int e = 0; e < 8; ++e) stf(out + e * 16, acc[e]);
  }
}

// dgamma[c, j<3H] = sum_bt dpre[bt, c, pi(j)] * xg[bt, j]
// dbeta4[c, j<4H] = sum_bt dpre[bt, c, pi(j)]   (slice 2, d_hhn -> db_hh_n)
// grid.y slices BT; f32 atomics finalize.  Natural-order outputs.
// xg_pi is the pi-permuted xg image: one ld8 per bt instead of 8 scalars.
template <typename T>
__global__ void gru_dgamma_kernel(const T* __restrict__ dpre,   // (BT, C, 4H) pi
                                  const T* __restrict__ xg_pi,  // (BT, 3H) pi
                                  float* __restrict__ dgamma,   // (C, 3H) zeroed
                                  float* __restrict__ dbeta4,   // (C, 4H) zeroed
                                  int64_t BT, int C) {
  const int n_threads_needed = C * 64;   // 4 gates x 16 c_col groups
  const int tid_g = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid_g >= n_threads_needed) return;
  const int c = tid_g / 64;
  const int rem = tid_g % 64;
  const int s = rem / 16;                // dpre slice
  const int cc = rem % 16;
  const int g = gate_of_slice(s);
  const bool has_x = g >= 0;
  const int pi0 = s * H + cc * 8;        // in the dpre row
  const int xpi0 = g * H + cc * 8;       // in the xg_pi row (has_x only)
  const int64_t bt_lo = BT * blockIdx.y / gridDim.y;
  const int64_t bt_hi = BT * (blockIdx.y + 1) / gridDim.y;
  float accg[8], accb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { accg[e] = 0.f; accb[e] = 0.f; }
  // 4x unroll over bt for memory-level parallelism (see gru_dxg_kernel)
  int64_t bt = bt_lo;
  for (; bt + 4 <= bt_hi; bt += 4) {
    float d[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      ld8(dpre + ((bt + u) * C + c) * G4H + pi0, d[u]);
    if (has_x) {
      float xv[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        ld8(xg_pi + (bt + u) * G3H + xpi0, xv[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) accg[e] += d[u][e] * xv[u][e];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e) accb[e] += d[u][e];
  }
  for (; bt < bt_hi; ++bt) {
    float d[8];
    ld8(dpre + (bt * C + c) * G4H + pi0, d);
    if (has_x) {
      float xv[8];
      ld8(xg_pi + bt * G3H + xpi0, xv);
#pragma unroll
      for (int e = 0; e < 8; ++e) accg[e] += d[e] * xv[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) accb[e] += d[e];
  }
  float* b_out = dbeta4 + (int64_t)c * G4H + s * H + cc;
#pragma unroll
  for (int e = 0; e < 8; ++e) atomicAdd(b_out + e * 16, accb[e]);
  if (has_x) {
    float* g_out = dgamma + (int64_t)c * G3H + g * H + cc;
#pragma unroll
    for (int e = 0; e < 8; ++e) atomicAdd(g_out + e * 16, accg[e]);
  }
}

// ---- single pass: dxg, dgamma and dbeta4 from ONE read of each dpre row ----
// A workgroup of RF_WAVES waves owns a contiguous slab of bt rows and all C
// components.  One wave reads one whole row (lane = slice x 8-column chunk,
// 16 B per lane in bf16), and wave w owns components {w, w + RF_WAVES, ...},
// CPT of them, so its dgamma / dbeta4 partials stay in registers over the
// slab and leave the block once, as f32 atomics.  For dxg each lane pre-sums
// its own components times their gamma_pi rows (staged in LDS once per
// block); the RF_WAVES partial rows meet in a double-buffered LDS area (one
// barrier per bt, no atomics in the loop) and the first 384 threads store
// the dxg row contiguously in natural order.  The next bt's rows are in
// flight while the current one is consumed.
constexpr int REDUCE_FUSED_MAX_C = 64;   // RF_WAVES x the largest CPT
constexpr int RF_WAVES = 8;
constexpr int RF_GSTR = H + 16;          // partial-row gate stride: the two
                                         // slices of a half-wave hit
                                         // different LDS banks
constexpr int RF_PSTR = 3 * RF_GSTR;     // one wave's partial dxg row (f32)

template <typename T, int CPT>
struct ReduceLds {
  static constexpr int GAM = 0;          // (RF_WAVES*CPT, 3H) T, pi layout
  static constexpr int PART = GAM + RF_WAVES * CPT * G3H * (int)sizeof(T);
  static constexpr int TOTAL = PART + 2 * RF_WAVES * RF_PSTR * 4;
  static_assert(TOTAL <= LDS_MAX, "reduce LDS layout exceeds a workgroup's LDS");
};

// 8 values as loaded (bf16: 4 registers), converted only where consumed
template <typename T> struct Pack8;
template <> struct Pack8<uint16_t> { uint4 v; };
template <> struct Pack8<float> { float4 a, b; };
__device__ __forceinline__ void unpack8(const Pack8<uint16_t>& p, float* v) {
  const uint32_t w[4] = {p.v.x, p.v.y, p.v.z, p.v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void unpack8(const Pack8<float>& p, float* v) {
  v[0] = p.a.x; v[1] = p.a.y; v[2] = p.a.z; v[3] = p.a.w;
  v[4] = p.b.x; v[5] = p.b.y; v[6] = p.b.z; v[7] = p.b.w;
}

// raw buffer load of 8 values at a byte offset into a scalar descriptor
constexpr int BUF_RSRC_W3 = 0x00020000;  // gfx9 raw-buffer word 3: 32-bit data format
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
template <typename T>
__device__ __forceinline__ Pack8<T> ld_buf8(__amdgpu_buffer_rsrc_t r, uint32_t off);
template <>
__device__ __forceinline__ Pack8<uint16_t> ld_buf8<uint16_t>(__amdgpu_buffer_rsrc_t r,
                                                             uint32_t off) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return {make_uint4(v.x, v.y, v.z, v.w)};
}
template <>
__device__ __forceinline__ Pack8<float> ld_buf8<float>(__amdgpu_buffer_rsrc_t r,
                                                       uint32_t off) {
  const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  const u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(r, off + 16, 0, 0);
  return {make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z),
                      __uint_as_float(a.w)),
          make_float4(__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z),
                      __uint_as_float(b.w))};
}

// The 8 values exist in their own registers from here on, and nothing
// scheduled after this point moves before it: a refill issued next can land
// in the registers the values were unpacked from (no copy of the ring at the
// loop's back edge, which would wait for every load in flight).
__device__ __forceinline__ void take_out(float* v) {
#pragma unroll
  for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(v[e]));
  __builtin_amdgcn_sched_barrier(0);
}

// LDS-only workgroup barrier: waits for this wave's LDS traffic, not for its
// global loads, so the prefetched rows stay in flight across it
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <typename T, int CPT>
__global__ __launch_bounds__(RF_WAVES * DR_WAVE) void gru_reduce_fused_kernel(
    const T* __restrict__ dpre,      // (BT, C, 4H) pi: dr|dz|d_hhn|dn
    const T* __restrict__ gamma_pi,  // (C, 3H) pi
    const T* __restrict__ xg_pi,     // (BT, 3H) pi
    T* __restrict__ dxg,             // (BT, 3H)
    float* __restrict__ dgamma,      // (C, 3H) zeroed
    float* __restrict__ dbeta4,      // (C, 4H) zeroed, dpre's slice order
    int64_t BT, int C) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using L = ReduceLds<T, CPT>;
  using P = Pack8<T>;
  constexpr int NTHR = RF_WAVES * DR_WAVE;
  T* gam = reinterpret_cast<T*>(smem + L::GAM);
  float* part = reinterpret_cast<float*>(smem + L::PART);
  const int tid = threadIdx.x;
  // the wave index as a scalar: row addresses below are scalar base + lane
  const int w = __builtin_amdgcn_readfirstlane(tid / DR_WAVE);
  const int lane = tid % DR_WAVE;
  const int s = lane >> 4;               // dpre slice
  const int cc = lane & 15;
  const int g = gate_of_slice(s);
  const bool has_x = g >= 0;
  // d_hhn lanes run the x-side arithmetic on gate 0's operands and drop it
  // (no divergence inside the wave); they only keep dbeta4
  const int gx = has_x ? g : 0;

  // gamma_pi rows into LDS in 16-byte pieces; rows past C are zero
  constexpr int ROW16 = G3H * (int)sizeof(T) / 16;
  for (int id = tid; id < RF_WAVES * CPT * ROW16; id += NTHR) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (id / ROW16 < C) v = reinterpret_cast<const uint4*>(gamma_pi)[id];
    reinterpret_cast<uint4*>(gam)[id] = v;
  }
  __syncthreads();

  const int64_t bt_lo = BT * blockIdx.x / gridDim.x;
  const int64_t bt_hi = BT * (blockIdx.x + 1) / gridDim.x;
  float accg[CPT][8], accb[CPT][8];
#pragma unroll
  for (int k = 0; k < CPT; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) { accg[k][e] = 0.f; accb[k][e] = 0.f; }

  // Slots past C re-read component C - 1 (a valid row) against a zero gamma
  // row and are never flushed, and the last bt of the slab is re-read once
  // instead of ending the prefetch: every lane issues the same loads in
  // every iteration, so the wait counters stay exact and nothing drains the
  // rows in flight.
  uint32_t voff[CPT];                    // byte offset of slot k in a bt
#pragma unroll
  for (int k = 0; k < CPT; ++k)
    voff[k] = (uint32_t)min(w + k * RF_WAVES, C - 1) * (G4H * (uint32_t)sizeof(T)) +
              lane * 8 * (uint32_t)sizeof(T);
  const uint32_t xoff = (gx * H + cc * 8) * (uint32_t)sizeof(T);
  const T* grow = gam + w * G3H + gx * H + cc * 8;
  float* pw = part + w * RF_PSTR + gx * RF_GSTR + cc;
  const float* pr = part + (tid >> 7) * RF_GSTR + (tid & (H - 1));   // tid < 3H

  // Buffer loads: a scalar descriptor per bt (base and size of that bt's C
  // rows) + one 32-bit lane offset per slot.  With plain pointers the loop
  // optimizer keeps a 64-bit vector address per slot and CPT = 8 spills.
  auto row_base = [&](int64_t bt) {
    return __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T*>(dpre + bt * C * G4H), 0, C * G4H * (int)sizeof(T), BUF_RSRC_W3);
  };
  auto ld_row = [&](__amdgpu_buffer_rsrc_t base, int k) { return ld_buf8<T>(base, voff[k]); };
  auto ld_x = [&](int64_t bt) {
    return ld_buf8<T>(__builtin_amdgcn_make_buffer_rsrc(
                          const_cast<T*>(xg_pi + bt * G3H), 0, G3H * (int)sizeof(T),
                          BUF_RSRC_W3),
                      xoff);
  };

  // A ring of CPT rows (+ the xg row): each register set is refilled with
  // the next bt's row as soon as this bt's row has been taken out of it, so
  // one bt of rows per wave is in flight at any time.
  P ring[CPT], xring;
  if (bt_lo < bt_hi) {
    // same issue order as in the loop: the wait counts at its head then hold
    // for the first iteration and for the back edge alike
    xring = ld_x(bt_lo);
    const auto base = row_base(bt_lo);
#pragma unroll
    for (int k = 0; k < CPT; ++k) ring[k] = ld_row(base, k);
  }
  int boff = 0;                          // partial buffer of this bt
  for (int64_t bt = bt_lo; bt < bt_hi; ++bt) {
    const int64_t bt_n = bt + 1 < bt_hi ? bt + 1 : bt;
    const auto base_n = row_base(bt_n);
    float xv[8], px[8];
    unpack8(xring, xv);
    take_out(xv);
    xring = ld_x(bt_n);
#pragma unroll
    for (int e = 0; e < 8; ++e) px[e] = 0.f;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      float d[8], gm[8];
      unpack8(ring[k], d);
      take_out(d);
      ring[k] = ld_row(base_n, k);
      unpack8(*reinterpret_cast<const P*>(grow + k * RF_WAVES * G3H), gm);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        accb[k][e] += d[e];
        accg[k][e] += d[e] * xv[e];
        px[e] += d[e] * gm[e];
      }
      // pin this slot's sums here: left alone the optimizer unpacks every
      // slot first and sinks all the arithmetic below the last refill, and
      // the CPT x 8 live values spill to scratch
#pragma unroll
      for (int e = 0; e < 8; ++e)
        asm volatile("" : "+v"(accb[k][e]), "+v"(accg[k][e]), "+v"(px[e]));
      __builtin_amdgcn_sched_barrier(0);
    }
    if (has_x) {
#pragma unroll
      for (int e = 0; e < 8; ++e) pw[boff + e * 16] = px[e];   // natural column cc + 16e
    }
    // this buffer is rewritten two bt later, behind the NEXT barrier, which
    // every reader of it has passed by then
    lds_barrier();
    if (tid < G3H) {
      float sum = 0.f;
#pragma unroll
      for (int ww = 0; ww < RF_WAVES; ++ww) sum += pr[boff + ww * RF_PSTR];
      stf(dxg + bt * G3H + tid, sum);
    }
    boff ^= RF_WAVES * RF_PSTR;
  }

#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int c = w + k * RF_WAVES;
    if (c >= C) continue;
    float* b_out = dbeta4 + (int64_t)c * G4H + s * H + cc;
#pragma unroll
    for (int e = 0; e < 8; ++e) atomicAdd(b_out + e * 16, accb[k][e]);
    if (has_x) {
      float* g_out = dgamma + (int64_t)c * G3H + g * H + cc;
#pragma unroll
      for (int e = 0; e < 8; ++e) atomicAdd(g_out + e * 16, accg[k][e]);
    }
  }
}

// ------------------------------------------------------------- launchers
// TypeTag / with_io_type / allow_lds and the status convention: launch.h.

// The forward kernel's tile variant, chosen once for the sequence and the
// decode entry: f(FwdTile<FP8, NSUB>).
template <bool FP8_, int NSUB_> struct FwdTile {
  static constexpr bool FP8 = FP8_;
  static constexpr int NSUB = NSUB_;
};
template <typename F>
static hipError_t with_fwd_tile(int B, int C, int fp8, F&& f) {
  const int64_t tiles128 = ((int64_t)B * C + 2 * ROWS - 1) / (2 * ROWS);
  // 8-wave 128-row variant: 2 waves/SIMD.  It needs enough tiles to fill the
  // chip at one block per CU, and C >= 5: a wave's 16 rows must not span more
  // than its 4 xg staging slots (C = 4 spans up to 5 batch indices).
  const bool wide = !fp8 && tiles128 >= 192 && C >= 5;
  if (!wide && !fp8) return f(FwdTile<false, 1>{});
  if (fp8) return f(FwdTile<true, 1>{});
  return f(FwdTile<false, 2>{});
}
// Whether the training forward (SAVE) runs the head phase in the kernel: on
// the 8-wave tile only (its 4-wave twin spills).  The one place that decides;
// the sequence entry and dr_gru_fwd_fuses_heads both ask here.
template <typename Tile>
static constexpr bool fwd_train_heads(Tile) { return !Tile::FP8 && Tile::NSUB == 2; }

// Fills the operand-image buffer (see OperandImages) on the stream.
template <typename T>
static hipError_t operand_images_launch(const void* gamma, const void* beta,
                                        const float* b_hh, void* images, int C,
                                        hipStream_t stream) {
  if (images == nullptr) return hipErrorInvalidValue;
  using I = OperandImages<T>;
  char* img = static_cast<char*>(images);
  const int n = (2 * C + 1) * 48;
  hipLaunchKernelGGL((gru_operand_images_kernel<T>), dim3((n + 255) / 256), dim3(256),
                     0, stream, (const T*)gamma, (const T*)beta, b_hh,
                     (T*)(img + I::gamma(C)), (T*)(img + I::beta(C)),
                     (float*)(img + I::bhh(C)), C);
  return hipGetLastError();
}

struct FwdArgs {
  const void *xg, *gamma, *beta, *w_gemm;
  const float* b_hh;
  const void* h0;
  void *h_all, *saves;     // sequence entry (saves: SAVE only); decode: null
  int B, TT, C, reverse;
  const void* wh_fwd;      // head phase (decode, SAVE+HEADS); otherwise null / 0
  void *out, *h_last;      // h_last: decode entry only
  int O;
  const int* lens;         // VARLEN only
  void* images;            // operand-image buffer (streaming variants fill it)
  hipStream_t stream;
};

template <typename T, bool SAVE, bool FP8, int NSUB, bool HEADS, bool VARLEN>
static hipError_t gru_fwd_launch(const FwdArgs& a) {
  constexpr int LDS = FwdLds<FP8, NSUB, HEADS>::TOTAL;
  static const hipError_t attr =
      allow_lds(&gru_fwd_kernel<T, SAVE, FP8, NSUB, HEADS, VARLEN>, LDS);
  if (attr != hipSuccess) return attr;
  const int64_t R = (int64_t)a.B * a.C;
  const int grid = (int)((R + ROWS * NSUB - 1) / (ROWS * NSUB));
  const void *gamma = a.gamma, *beta = a.beta;
  const float* b_hh = a.b_hh;
  if constexpr (!fwd_gb_regs<FP8, NSUB, VARLEN>) {
    // the streaming variants read the pi-ordered images instead
    if (hipError_t e = operand_images_launch<T>(a.gamma, a.beta, a.b_hh, a.images,
                                                a.C, a.stream))
      return e;
    using I = OperandImages<T>;
    const char* img = static_cast<const char*>(a.images);
    gamma = img + I::gamma(a.C);
    beta = img + I::beta(a.C);
    b_hh = reinterpret_cast<const float*>(img + I::bhh(a.C));
  }
  hipLaunchKernelGGL((gru_fwd_kernel<T, SAVE, FP8, NSUB, HEADS, VARLEN>),
                     dim3(grid), dim3(THREADS * NSUB), LDS, a.stream,
                     (const T*)a.xg, (const T*)gamma, (const T*)beta,
                     (const uint16_t*)a.w_gemm, b_hh, (const T*)a.h0,
                     (T*)a.h_all, (T*)a.saves, a.B, a.TT, a.C, a.reverse,
                     (const uint16_t*)a.wh_fwd, (T*)a.out, (T*)a.h_last, a.O,
                     a.lens);
  return hipGetLastError();
}

struct BwdArgs {
  const void *grad, *wh_img, *w_img, *w_fwd, *xg, *gamma, *beta;
  const float* b_hh;
  const void *h0, *h_all, *saves;
  void* dpre;
  float* dh0;
  int B, TT, C, reverse, O;
  void* images;            // operand-image buffer, filled here
  hipStream_t stream;
};

template <typename T, int NSUB, bool FUSED>
static hipError_t gru_bwd_launch(const BwdArgs& a) {
  constexpr int LDS = BwdLds<NSUB, FUSED>::TOTAL;
  static const hipError_t attr =
      LDS ? allow_lds(&gru_bwd_kernel<T, NSUB, FUSED>, LDS) : hipSuccess;
  if (attr != hipSuccess) return attr;
  const int64_t R = (int64_t)a.B * a.C;
  const int grid = (int)((R + ROWS * NSUB - 1) / (ROWS * NSUB));
  // gamma / beta reach the kernel as pi-ordered images; b_hh stays natural
  // (its n slice sits in registers over the whole loop)
  if (hipError_t e = operand_images_launch<T>(a.gamma, a.beta, a.b_hh, a.images,
                                              a.C, a.stream))
    return e;
  using I = OperandImages<T>;
  const char* img = static_cast<const char*>(a.images);
  hipLaunchKernelGGL((gru_bwd_kernel<T, NSUB, FUSED>), dim3(grid),
                     dim3(THREADS * NSUB), LDS, a.stream, (const T*)a.grad,
                     (const uint16_t*)a.wh_img, (const uint16_t*)a.w_img,
                     (const uint16_t*)a.w_fwd, (const T*)a.xg,
                     (const T*)(img + I::gamma(a.C)), (const T*)(img + I::beta(a.C)),
                     a.b_hh,
                     (const T*)a.h0, (const T*)a.h_all, (const T*)a.saves,
                     (T*)a.dpre, a.dh0, a.B, a.TT, a.C, a.reverse, a.O);
  return hipGetLastError();
}

// compute units of the current device, asked once per process (see allow_lds)
static int cu_count() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      n <= 0)
    n = 256;
  return n;
}

template <typename T, int CPT>
static hipError_t gru_reduce_fused_launch(const T* dpre, const T* gamma_pi,
                                          const T* xg_pi, T* dxg, float* dgamma,
                                          float* dbeta, int64_t BT, int C,
                                          hipStream_t stream) {
  constexpr int LDS = ReduceLds<T, CPT>::TOTAL;
  static const hipError_t attr = allow_lds(&gru_reduce_fused_kernel<T, CPT>, LDS);
  if (attr != hipSuccess) return attr;
  // one resident block per CU, each flushing its dgamma / dbeta4 partials once
  static const int n_cu = cu_count();
  const int grid = (int)std::min<int64_t>(BT, n_cu);
  hipLaunchKernelGGL((gru_reduce_fused_kernel<T, CPT>), dim3(grid),
                     dim3(RF_WAVES * DR_WAVE), LDS, stream, dpre, gamma_pi, xg_pi,
                     dxg, dgamma, dbeta, BT, C);
  return hipGetLastError();
}

enum ReduceMode { REDUCE_AUTO = 0, REDUCE_SPLIT = 1, REDUCE_FUSED = 2 };

template <typename T>
static hipError_t gru_reduce_launch(const void* dpre, const void* gamma,
                                    const void* xg, void* dxg, float* dgamma,
                                    float* dbeta, void* gamma_pi, void* xg_pi,
                                    int64_t BT, int C, int mode,
                                    hipStream_t stream) {
  if (BT <= 0 || C <= 0) return hipErrorInvalidValue;
  if (mode == REDUCE_FUSED && C > REDUCE_FUSED_MAX_C) return hipErrorInvalidValue;
  const bool fused = mode == REDUCE_FUSED ||
                     (mode == REDUCE_AUTO && C <= REDUCE_FUSED_MAX_C);
  auto chunk_grid = [](int64_t rows) {
    return (int)std::min<int64_t>((rows * 48 + 255) / 256, 4096);
  };
  // stage pi-layout images of gamma and xg (once per backward, ~47 MB at
  // bench scale) so the reduction inner loops are pure 16-byte loads
  hipLaunchKernelGGL((pi_permute_rows_kernel<T>), dim3(chunk_grid(C)), dim3(256),
                     0, stream, (const T*)gamma, (T*)gamma_pi, (int64_t)C);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL((pi_permute_rows_kernel<T>), dim3(chunk_grid(BT)), dim3(256),
                     0, stream, (const T*)xg, (T*)xg_pi, BT);
  if (hipError_t e = hipGetLastError()) return e;
  if (fused) {
    auto run = [&](auto cpt) {
      return gru_reduce_fused_launch<T, decltype(cpt)::value>(
          (const T*)dpre, (const T*)gamma_pi, (const T*)xg_pi, (T*)dxg, dgamma,
          dbeta, BT, C, stream);
    };
    const int need = (C + RF_WAVES - 1) / RF_WAVES;   // components per wave
    if (need <= 1) return run(std::integral_constant<int, 1>{});
    if (need <= 2) return run(std::integral_constant<int, 2>{});
    if (need <= 4) return run(std::integral_constant<int, 4>{});
    return run(std::integral_constant<int, 8>{});
  }
  hipLaunchKernelGGL((gru_dxg_kernel<T>), dim3(chunk_grid(BT)), dim3(256), 0,
                     stream, (const T*)dpre, (const T*)gamma_pi, (T*)dxg, BT, C);
  if (hipError_t e = hipGetLastError()) return e;
  const int gx = (C * 64 + 255) / 256;
  const int gy = 128;  // BT slices (parallelism for small C; atomics stay cheap)
  hipLaunchKernelGGL((gru_dgamma_kernel<T>), dim3(gx, gy), dim3(256), 0, stream,
                     (const T*)dpre, (const T*)xg_pi, dgamma, dbeta, BT, C);
  return hipGetLastError();
}

}  // namespace dr

extern "C" {

// Entry contracts: kernels.h.

int64_t dr_gru_operand_images_bytes(int C, int is_bf16) {
  return is_bf16 ? dr::OperandImages<uint16_t>::total(C)
                 : dr::OperandImages<float>::total(C);
}

int dr_gru_fwd_fuses_heads(int B, int C) {
  bool fuses = false;
  (void)dr::with_fwd_tile(B, C, 0, [&](auto tile) {
    fuses = dr::fwd_train_heads(tile);
    return hipSuccess;
  });
  return fuses ? 1 : 0;
}

int dr_gru_fwd(const void* xg, const void* gamma, const void* beta,
               const void* w_hh, const float* b_hh, const void* h0, void* h_all,
               void* saves, const void* wh_fwd, void* out, int O, int B, int TT,
               int C, int reverse, int save, int fp8, int is_bf16,
               void* images, hipStream_t stream) {
  const bool heads = wh_fwd != nullptr;
  const dr::FwdArgs a{xg, gamma, beta, w_hh, b_hh, h0, h_all, saves, B, TT, C,
                      reverse, wh_fwd, out, nullptr, heads ? O : 0, nullptr, images,
                      stream};
  if (heads && !save) return (int)hipErrorInvalidValue;
  return (int)dr::with_io_type(is_bf16, [&](auto io) {
    using T = typename decltype(io)::type;
    return dr::with_fwd_tile(B, C, fp8, [&](auto tile) {
      using V = decltype(tile);
      if constexpr (dr::fwd_train_heads(V{})) {
        if (heads) return dr::gru_fwd_launch<T, true, false, V::NSUB, true, false>(a);
      } else {
        if (heads) return hipErrorInvalidValue;
      }
      // the fp8 tiles are inference-only: no SAVE instantiation exists
      if constexpr (!V::FP8)
        if (save) return dr::gru_fwd_launch<T, true, false, V::NSUB, false, false>(a);
      return dr::gru_fwd_launch<T, false, V::FP8, V::NSUB, false, false>(a);
    });
  });
}

int dr_gru_decode(const void* xg, const void* gamma, const void* beta,
                  const void* w_hh, const float* b_hh, const void* h0,
                  const void* wh_fwd, void* out, void* h_last, int B, int TT,
                  int C, int O, int reverse, int fp8, int is_bf16,
                  const int* lens, void* images, hipStream_t stream) {
  const dr::FwdArgs a{xg, gamma, beta, w_hh, b_hh, h0, nullptr, nullptr, B, TT, C,
                      reverse, wh_fwd, out, h_last, O, lens, images, stream};
  auto run = [&](auto varlen) {
    return dr::with_io_type(is_bf16, [&](auto io) {
      using T = typename decltype(io)::type;
      return dr::with_fwd_tile(B, C, fp8, [&](auto tile) {
        using V = decltype(tile);
        return dr::gru_fwd_launch<T, false, V::FP8, V::NSUB, true,
                                  decltype(varlen)::value>(a);
      });
    });
  };
  return (int)(lens != nullptr ? run(std::true_type{}) : run(std::false_type{}));
}

int dr_gru_bwd(const void* grad, const void* wh_img, int O, const void* w_img,
               const void* w_fwd, const void* xg, const void* gamma,
               const void* beta, const float* b_hh, const void* h0,
               const void* h_all, const void* saves, void* dpre, float* dh0,
               int B, int TT, int C, int reverse, int is_bf16, void* images,
               hipStream_t stream) {
  const bool fused = wh_img != nullptr;
  const dr::BwdArgs a{grad, wh_img, w_img, w_fwd, xg, gamma, beta, b_hh, h0,
                      h_all, saves, dpre, dh0, B, TT, C, reverse, fused ? O : 0,
                      images, stream};
  // enough 128-row tiles to fill the chip at 1 block/CU: the LDS-W variant
  const int64_t tiles128 = ((int64_t)B * C + 2 * dr::ROWS - 1) / (2 * dr::ROWS);
  const bool lds_w = tiles128 >= 192;
  auto run = [&](auto fused_tag) {
    return dr::with_io_type(is_bf16, [&](auto io) {
      using T = typename decltype(io)::type;
      constexpr bool FUSED = decltype(fused_tag)::value;
      return lds_w ? dr::gru_bwd_launch<T, 2, FUSED>(a)
                   : dr::gru_bwd_launch<T, 1, FUSED>(a);
    });
  };
  return (int)(fused ? run(std::true_type{}) : run(std::false_type{}));
}

int dr_gru_reduce_fused_max_c() { return dr::REDUCE_FUSED_MAX_C; }

int dr_gru_bwd_reduce(const void* dpre, const void* gamma, const void* xg,
                      void* dxg, float* dgamma, float* dbeta, void* gamma_pi,
                      void* xg_pi, int64_t BT, int C, int mode, int is_bf16,
                      hipStream_t stream) {
  return (int)dr::with_io_type(is_bf16, [&](auto io) {
    using T = typename decltype(io)::type;
    return dr::gru_reduce_launch<T>(dpre, gamma, xg, dxg, dgamma, dbeta,
                                    gamma_pi, xg_pi, BT, C, mode, stream);
  });
}

}  // extern "C"
