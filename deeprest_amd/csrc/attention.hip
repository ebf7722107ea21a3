// Fused multi-head attention for gfx950 (MFMA), forward and backward.
//
// Two sets of bodies behind one launcher (mha_whole_tile, near the end): the
// whole-head tile kernels for T <= 64, and the flash-style kernels below for
// everything else.  All of them address q, k, v, o by (batch, head, time)
// element strides, so they run on (B, H, T, D) tensors and on the packed qkv
// projection (B, T, 3, H, D) alike.
//
// Flash-style forward: one workgroup (4 waves) per 64-row Q tile of one
// (batch, head): QK^T on v_mfma_f32_16x16x32_bf16 with the K tile staged in
// LDS (rows padded +16 B
// so the 16-lane ds_read_b128 groups land on distinct banks), online softmax
// entirely in registers (running row max/denominator, rescale-on-grow), PV
// on MFMA with V staged transposed.  No S x S score tensor ever exists in
// memory; the per-row logsumexp is saved for the recompute backward
// (deeprest_amd/ops/attention.py).
//
// Internal compute is bf16 MFMA with fp32 softmax statistics and fp32 O
// accumulation; fp32 inputs are rounded to bf16 at the MFMA operands only.
// Head dims supported: 8 <= D <= 64, D % 8 == 0 (the traffic encoder uses
// D = d_model / n_heads = 32).
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace dr {

constexpr int QT = 64;     // Q rows per block
constexpr int KT_KEYS = 32;  // keys per tile
constexpr int A_WAVES = 4;
constexpr int A_THREADS = A_WAVES * DR_WAVE;
constexpr int DMAX = 64;
// padded LDS row strides (bytes): +16 B breaks the power-of-2 bank pattern
constexpr int K_STRIDE = DMAX * 2 + 16;      // K tile: [key][d]
constexpr int V_STRIDE = KT_KEYS * 2 + 16;   // V^T tile: [d][key]
constexpr int P_STRIDE = KT_KEYS * 2 + 16;   // P tile:  [qrow][key]

// Element strides of a (batch, head, time, d) operand with unit d stride.
// (B, H, T, D) contiguous: {H*T*D, T*D, D}; the q / k / v parts of a packed
// (B, T, 3, H, D) qkv: {T*3*H*D, D, 3*H*D}; a (B, T, H*D) output: {T*H*D, D, H*D}.
struct MhaStrides {
  int64_t sb, sh, st;
};

// VARLEN = true (inference only): sample b = bh / n_heads is valid at
// t < L = clamp(kv_len[b], 1, T_len).  Keys >= L are absent (never staged,
// never scored), query tiles at or past L store zeros and leave before the
// first barrier, rows >= L of a partly valid tile store zeros.  Strides keep
// using T_len.
template <typename T, bool VARLEN = false>
__global__ __launch_bounds__(A_THREADS) void mha_fwd_kernel(
    const T* __restrict__ q,   // element (b, h, t, d) at b*sb + h*sh + t*st + d
    const T* __restrict__ k,
    const T* __restrict__ v,
    T* __restrict__ o,         // same, with the strides `os`
    float* __restrict__ lse,   // (BH, T)
    MhaStrides qs, MhaStrides os,
    int T_len, int D, float scale,
    const int* __restrict__ kv_len,  // VARLEN: (B,) int32
    int n_heads) {
  __shared__ __attribute__((aligned(16))) char k_lds[KT_KEYS * K_STRIDE];
  __shared__ __attribute__((aligned(16))) char vt_lds[DMAX * V_STRIDE];
  __shared__ __attribute__((aligned(16))) char p_lds[QT * P_STRIDE];

  const int tid = threadIdx.x;
  const int wv = tid / DR_WAVE;
  const int lane = tid % DR_WAVE;
  const int64_t bh = blockIdx.y;
  const int q0 = blockIdx.x * QT;

  const int64_t in_off = (bh / n_heads) * qs.sb + (bh % n_heads) * qs.sh;
  const T* qb = q + in_off;
  const T* kb = k + in_off;
  const T* vb = v + in_off;
  T* ob = o + (bh / n_heads) * os.sb + (bh % n_heads) * os.sh;

  const int c_col = lane & 15;
  const int rgrp = lane >> 4;

  // valid length of this block's sample: T_len itself without VARLEN
  int L = T_len;
  if constexpr (VARLEN) {
    L = std::min(std::max(kv_len[blockIdx.y / n_heads], 1), T_len);
    if (q0 >= L) {                       // block-uniform: a fully padded tile
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int row = q0 + wv * 16 + rgrp * 4 + i;
        if (row >= T_len) continue;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          int d = nt * 16 + c_col;
          if (d < D) stf(ob + (int64_t)row * os.st + d, 0.f);
        }
        if (c_col == 0) lse[bh * T_len + row] = 0.f;
      }
      return;
    }
  }

  // ---- Q fragments: this wave's 16 rows, zero-padded past D and L ----
  const int n_kt_qk = (D + 31) / 32;  // K-tiles in QK^T (K dim = D)
  bf16x8 qfrag[2];
  {
    const int qrow = q0 + wv * 16 + (lane & 15);
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      uint16_t tmp[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int d = kt * 32 + rgrp * 8 + j;
        float val = (qrow < L && d < D) ? ldf(qb + (int64_t)qrow * qs.st + d) : 0.f;
        tmp[j] = f2bf(val);
      }
      qfrag[kt] = *reinterpret_cast<bf16x8*>(tmp);
    }
  }

  // ---- per-row online softmax state (4 rows per lane, C-layout) ----
  // o_acc[nt] is the MFMA C fragment of output d-tile nt: element i = row
  // sub-index (row = (lane>>4)*4 + i), col = nt*16 + (lane&15).
  float m_run[4], l_run[4];
  f32x4 o_acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { m_run[i] = -1e30f; l_run[i] = 0.f; }
  const int n_d_tiles = (D + 15) / 16;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int e = 0; e < 4; ++e) o_acc[nt][e] = 0.f;

  const int n_key_tiles = (L + KT_KEYS - 1) / KT_KEYS;
  for (int ktile = 0; ktile < n_key_tiles; ++ktile) {
    const int key0 = ktile * KT_KEYS;

    // ---- cooperative stage: K tile [key][d], V^T tile [d][key] ----
    __syncthreads();  // previous iteration's reads done
    for (int id = tid; id < KT_KEYS * (DMAX / 8); id += A_THREADS) {
      int key = id / (DMAX / 8);
      int blk = id % (DMAX / 8);
      uint16_t* dst = reinterpret_cast<uint16_t*>(k_lds + key * K_STRIDE + blk * 16);
      int krow = key0 + key;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int d = blk * 8 + e;
        dst[e] = f2bf((krow < L && d < D) ? ldf(kb + (int64_t)krow * qs.st + d) : 0.f);
      }
    }
    for (int id = tid; id < DMAX * KT_KEYS / 8; id += A_THREADS) {
      int d = id / (KT_KEYS / 8);
      int kb8 = id % (KT_KEYS / 8);
      uint16_t* dst = reinterpret_cast<uint16_t*>(vt_lds + d * V_STRIDE + kb8 * 16);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int key = key0 + kb8 * 8 + e;
        dst[e] = f2bf((key < L && d < D) ? ldf(vb + (int64_t)key * qs.st + d) : 0.f);
      }
    }
    __syncthreads();

    // ---- S = Q K^T * scale for this wave's 16 rows x 32 keys ----
    f32x4 s_acc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {  // compile-time index (rule 20)
        if (kt >= n_kt_qk) continue;
        // B operand: K^T -> B[dk][key]: lane col = key (16-wide), k = d
        int key = nt * 16 + c_col;
        int d0 = kt * 32 + rgrp * 8;
        bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
            k_lds + key * K_STRIDE + d0 * 2);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfrag[kt], bfrag, a, 0, 0, 0);
      }
      s_acc[nt] = a;
    }

    // ---- online softmax (per lane: 4 rows x 2 key-cols) ----
    float p[2][4];
    float pmax[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pmax[i] = -1e30f;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      int key = key0 + nt * 16 + c_col;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s = (key < L) ? s_acc[nt][i] * scale : -1e30f;
        p[nt][i] = s;
        pmax[i] = fmaxf(pmax[i], s);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pmax[i] = group16_max(pmax[i]);
      float m_new = fmaxf(m_run[i], pmax[i]);
      float alpha = __expf(m_run[i] - m_new);  // m_run starts -1e30 -> alpha 0
      m_run[i] = m_new;
      l_run[i] *= alpha;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) o_acc[nt][i] *= alpha;
    }
    // exponentiate + row sums (per-wave 16-lane col groups)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 4; ++i) p[nt][i] = __expf(p[nt][i] - m_run[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      l_run[i] += group16_sum(p[0][i] + p[1][i]);
    // P -> bf16 -> LDS (this wave's own rows; wave-coherent, no barrier)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      int keyc = nt * 16 + c_col;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int row = wv * 16 + rgrp * 4 + i;
        *reinterpret_cast<uint16_t*>(p_lds + row * P_STRIDE + keyc * 2) =
            f2bf(p[nt][i]);
      }
    }

    // ---- O += P V  (A = P from LDS, B = V^T from LDS) ----
    {
      bf16x8 pfrag;
      int prow = wv * 16 + (lane & 15);
      pfrag = *reinterpret_cast<const bf16x8*>(
          p_lds + prow * P_STRIDE + (rgrp * 8) * 2);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {  // compile-time index (rule 20)
        if (nt >= n_d_tiles) continue;
        int d = nt * 16 + c_col;
        bf16x8 vfrag = *reinterpret_cast<const bf16x8*>(
            vt_lds + d * V_STRIDE + (rgrp * 8) * 2);
        o_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            pfrag, vfrag, o_acc[nt], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: O / l, store O and lse ----
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int row = q0 + wv * 16 + rgrp * 4 + i;
    if (row >= T_len) continue;
    float inv_l = (l_run[i] > 0.f) ? 1.f / l_run[i] : 0.f;
    // VARLEN: rows >= L of a partly valid tile store exact zeros (a select:
    // whatever the padded q row produced never reaches memory)
    const bool pad = VARLEN && row >= L;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {  // compile-time index (rule 20)
      if (nt >= n_d_tiles) continue;
      int d = nt * 16 + c_col;
      if (d < D)
        stf(ob + (int64_t)row * os.st + d, pad ? 0.f : o_acc[nt][i] * inv_l);
    }
    if (c_col == 0)
      lse[bh * T_len + row] =
          pad ? 0.f : m_run[i] + __logf(fmaxf(l_run[i], 1e-30f));
  }
}

// ---------------------------------------------------------------- backward
// Flash-style: one block per (bh, 64-key tile), 4 waves x 16 keys each.
// Everything key-indexed (S^T, dP^T, dS^T) accumulates in the SAME MFMA
// C-layout — key rows per lane, q columns per 16-lane group — so the
// softmax-gradient elementwise math is entirely lane-local with per-column
// lse / D_row reads.  dK/dV accumulate in registers (exclusive key rows);
// dQ contributions scatter with fp32 atomics (few per block at these T).
template <typename T>
__global__ __launch_bounds__(A_THREADS) void mha_bwd_kernel(
    const T* __restrict__ q,    // strides qs (as in mha_fwd_kernel)
    const T* __restrict__ k,
    const T* __restrict__ v,
    const T* __restrict__ o,    // strides os
    const T* __restrict__ dout, // strides os
    const float* __restrict__ lse,   // (BH, T)
    float* __restrict__ dq,          // strides dqs, fp32 (atomic accumulate)
    T* __restrict__ dk,              // strides qs
    T* __restrict__ dv,
    MhaStrides qs, MhaStrides os, MhaStrides dqs,
    int T_len, int D, float scale, int n_heads) {
  // LDS: q / do tiles (32 x D bf16, padded rows) + per-wave P/ds scratch +
  // per-q-tile lse/Drow
  __shared__ __attribute__((aligned(16))) char q_lds[32 * K_STRIDE];
  __shared__ __attribute__((aligned(16))) char do_lds[32 * K_STRIDE];
  __shared__ __attribute__((aligned(16))) char p_sc[A_WAVES * 16 * (32 * 2 + 16)];
  __shared__ float lse_s[32];
  __shared__ float drow_s[32];

  const int tid = threadIdx.x;
  const int wv = tid / DR_WAVE;
  const int lane = tid % DR_WAVE;
  const int64_t bh = blockIdx.y;
  const int key0 = blockIdx.x * 64 + wv * 16;  // this wave's 16 keys

  const int64_t bb = bh / n_heads, hh = bh % n_heads;
  const int64_t in_off = bb * qs.sb + hh * qs.sh;
  const int64_t o_off = bb * os.sb + hh * os.sh;
  const T* qb = q + in_off;
  const T* kb = k + in_off;
  const T* vb = v + in_off;
  const T* ob = o + o_off;
  const T* dob = dout + o_off;
  float* dqb = dq + bb * dqs.sb + hh * dqs.sh;
  T* dkb = dk + in_off;
  T* dvb = dv + in_off;

  const int c_col = lane & 15;
  const int rgrp = lane >> 4;
  const int n_kt_d = (D + 31) / 32;   // K-tiles over the D axis
  const int n_d_tiles = (D + 15) / 16;

  // ---- K and V fragments for this wave's 16 keys (A operands, row = key) ----
  bf16x8 kfrag[2], vfrag[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    uint16_t tk[8], tv[8];
    int krow = key0 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int d = kt * 32 + rgrp * 8 + j;
      bool ok = krow < T_len && d < D;
      tk[j] = f2bf(ok ? ldf(kb + (int64_t)krow * qs.st + d) : 0.f);
      tv[j] = f2bf(ok ? ldf(vb + (int64_t)krow * qs.st + d) : 0.f);
    }
    kfrag[kt] = *reinterpret_cast<bf16x8*>(tk);
    vfrag[kt] = *reinterpret_cast<bf16x8*>(tv);
  }

  // dK/dV accumulators: this wave's 16 key rows x D
  f32x4 dk_acc[4], dv_acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int e = 0; e < 4; ++e) { dk_acc[nt][e] = 0.f; dv_acc[nt][e] = 0.f; }

  const int PW_STRIDE = 32 * 2 + 16;           // bytes per scratch row
  char* my_p = p_sc + wv * 16 * PW_STRIDE;     // 16 key rows x 32 q cols

  const int n_qt = (T_len + 31) / 32;
  for (int qt = 0; qt < n_qt; ++qt) {
    const int q0 = qt * 32;
    // ---- cooperative stage: q / do tiles + lse + Drow ----
    __syncthreads();
    for (int id = tid; id < 32 * (DMAX / 8); id += A_THREADS) {
      int row = id / (DMAX / 8);
      int blk = id % (DMAX / 8);
      uint16_t* dstq = reinterpret_cast<uint16_t*>(q_lds + row * K_STRIDE + blk * 16);
      uint16_t* dstd = reinterpret_cast<uint16_t*>(do_lds + row * K_STRIDE + blk * 16);
      int qrow = q0 + row;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int d = blk * 8 + e;
        bool ok = qrow < T_len && d < D;
        dstq[e] = f2bf(ok ? ldf(qb + (int64_t)qrow * qs.st + d) : 0.f);
        dstd[e] = f2bf(ok ? ldf(dob + (int64_t)qrow * os.st + d) : 0.f);
      }
    }
    // Drow[r] = sum_d do[r,d] * o[r,d]; lse per row (one wave's worth of rows)
    if (tid < 32) {
      int qrow = q0 + tid;
      float s = 0.f;
      if (qrow < T_len) {
        for (int d = 0; d < D; ++d)
          s += ldf(dob + (int64_t)qrow * os.st + d) * ldf(ob + (int64_t)qrow * os.st + d);
        lse_s[tid] = lse[bh * T_len + qrow];
      } else {
        lse_s[tid] = 0.f;
      }
      drow_s[tid] = s;
    }
    __syncthreads();

    // ---- S^T = K Q^T * scale; P^T = exp(S^T - lse[col]) ----
    f32x4 st[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        if (kt >= n_kt_d) continue;
        // B operand: Q^T -> B[d][qcol]: lane col = q (16-wide), k = d
        int qc = nt * 16 + c_col;
        bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
            q_lds + qc * K_STRIDE + (kt * 32 + rgrp * 8) * 2);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag[kt], bfrag, a, 0, 0, 0);
      }
      st[nt] = a;
    }
    // dP^T = V dO^T (same structure)
    f32x4 dpt[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        if (kt >= n_kt_d) continue;
        int qc = nt * 16 + c_col;
        bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
            do_lds + qc * K_STRIDE + (kt * 32 + rgrp * 8) * 2);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfrag[kt], bfrag, a, 0, 0, 0);
      }
      dpt[nt] = a;
    }

    // ---- elementwise: P^T and dS^T (lane-local; cols give lse/Drow) ----
    // rows = keys (reg i), cols = q.  Write both into per-wave scratch:
    // P^T rows for the dV GEMM, then dS^T for the dK/dQ GEMMs.
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      int qc = nt * 16 + c_col;
      bool qok = (q0 + qc) < T_len;
      float l = lse_s[qc];
      float dr = drow_s[qc];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int key = key0 + rgrp * 4 + i;
        float p = 0.f, ds = 0.f;
        if (qok && key < T_len) {
          p = __expf(st[nt][i] * scale - l);
          ds = p * (dpt[nt][i] - dr) * scale;
        }
        int row = rgrp * 4 + i;
        *reinterpret_cast<uint16_t*>(my_p + row * PW_STRIDE + (nt * 16 + c_col) * 2) =
            f2bf(p);
        st[nt][i] = ds;  // reuse register: stash dS^T
      }
    }
    // dV += P^T dO   (A = P^T from scratch, B = dO tile read k-major)
    {
      bf16x8 pfrag;
      int prow = lane & 15;
      pfrag = *reinterpret_cast<const bf16x8*>(
          my_p + prow * PW_STRIDE + (rgrp * 8) * 2);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        if (nt >= n_d_tiles) continue;
        // B[qrow][d]: lane col = d, k = qrow -> read dO transposed: stride!
        // dO tile is row-major [q][d]; B operand needs contiguous q for a
        // fixed d — strided 8 reads (D*2 apart), packed here.
        uint16_t bq[8];
        int d = nt * 16 + c_col;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int qrow = rgrp * 8 + j;
          bq[j] = *reinterpret_cast<const uint16_t*>(
              do_lds + qrow * K_STRIDE + d * 2);
        }
        bf16x8 bfrag = *reinterpret_cast<bf16x8*>(bq);
        dv_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            pfrag, bfrag, dv_acc[nt], 0, 0, 0);
      }
    }
    // write dS^T into scratch, then dK += dS^T Q (same pattern as dV)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int row = rgrp * 4 + i;
        *reinterpret_cast<uint16_t*>(my_p + row * PW_STRIDE + (nt * 16 + c_col) * 2) =
            f2bf(st[nt][i]);
      }
    {
      bf16x8 dsfrag;
      int prow = lane & 15;
      dsfrag = *reinterpret_cast<const bf16x8*>(
          my_p + prow * PW_STRIDE + (rgrp * 8) * 2);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        if (nt >= n_d_tiles) continue;
        uint16_t bq[8];
        int d = nt * 16 + c_col;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int qrow = rgrp * 8 + j;
          bq[j] = *reinterpret_cast<const uint16_t*>(
              q_lds + qrow * K_STRIDE + d * 2);
        }
        bf16x8 bfrag = *reinterpret_cast<bf16x8*>(bq);
        dk_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            dsfrag, bfrag, dk_acc[nt], 0, 0, 0);
      }
    }
    // dQ[q0+qc][d] += sum over this wave's 16 keys of dS[qc,key] K[key,d]:
    // MFMA with A = dS (q rows x key cols) = transpose of scratch -> read
    // strided; B = K fragments ALREADY row=key (reuse via LDS? K is in regs
    // as A-layout) — do it with A = dS rows from scratch (strided pack) and
    // B[key][d] read from global k (L2).
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {  // two 16-row halves of the 32-q tile
      uint16_t aq[8];
      int qrow_l = qh * 16 + (lane & 15);  // q row within the tile
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int keyr = rgrp * 8 + j;
        aq[j] = keyr < 16 ? *reinterpret_cast<const uint16_t*>(
                                my_p + keyr * PW_STRIDE + qrow_l * 2)
                          : (uint16_t)0;
      }
      // wait: scratch holds only 32 q cols; qrow_l in 0..31 OK.
      // K dim = 32 but only this wave's 16 keys are real (upper half zeroed).
      bf16x8 afrag = *reinterpret_cast<bf16x8*>(aq);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        if (nt >= n_d_tiles) continue;
        uint16_t bk[8];
        int d = nt * 16 + c_col;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int keyr = rgrp * 8 + j;
          int krow = key0 + keyr;
          bool ok = keyr < 16 && krow < T_len && d < D;
          bk[j] = f2bf(ok ? ldf(kb + (int64_t)krow * qs.st + d) : 0.f);
        }
        bf16x8 bfrag = *reinterpret_cast<bf16x8*>(bk);
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag, bfrag, a, 0, 0, 0);
        // scatter-add into dq (fp32)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          int qrow = q0 + qh * 16 + rgrp * 4 + i;
          int d2 = nt * 16 + c_col;
          if (qrow < T_len && d2 < D)
            atomicAdd(dqb + (int64_t)qrow * dqs.st + d2, a[i]);
        }
      }
    }
  }

  // ---- store dK / dV (exclusive key rows) ----
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int krow = key0 + rgrp * 4 + i;
    if (krow >= T_len) continue;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      if (nt >= n_d_tiles) continue;
      int d = nt * 16 + c_col;
      if (d < D) {
        stf(dkb + (int64_t)krow * qs.st + d, dk_acc[nt][i]);
        stf(dvb + (int64_t)krow * qs.st + d, dv_acc[nt][i]);
      }
    }
  }
}

// ------------------------------------------------- whole head in one tile
// T <= 64: one WAVE holds all queries and all keys of one (batch, head), padded
// to 64 rows.  Every global access is one 16-byte piece of a (t, head) row per
// lane (f32 IO: two loads / one 16-byte store); an MFMA fragment of q, k, v or
// dO (row = lane & 15, 8 consecutive d) is that load itself.  A wave reads only
// LDS it wrote, so there is no block barrier: wave_lds_fence() orders the
// image stores ahead of the transposed reads.  The 4 waves of a block are 4
// independent heads.
//
// A score accumulator tile is the next product's B operand without leaving its
// lane: lane (c = lane & 15, g = lane >> 4) holds rows 4g .. 4g+3 of column c,
// so the two row tiles of a 32-row k-step give element j of the fragment the
// row perm(g, j) = 16 (j >> 2) + 4g + (j & 3).  The A operand follows that
// order: it is read with ds_read_b64_tr_b16 from a row-major [row][d] image,
// blocks of rows 16 jj + 4g .. + 3 (jj = j >> 2).  All 64 lanes issue every
// transposed read, with an in-bounds address of the padded image.
constexpr int TILE_T = 64;
constexpr int DS_STRIDE = 2 * TILE_T + 8;   // dS^T image row: [key][64 q] + 8 B

using s16x4 = __attribute__((ext_vector_type(4))) short;

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 8 consecutive elements as floats; ok == false: zeros, nothing is read
__device__ __forceinline__ void ld8f(const uint16_t* p, bool ok, float v[8]) {
  uint4 u = make_uint4(0u, 0u, 0u, 0u);
  if (ok) u = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = bf2f((uint16_t)(w[i] & 0xffff));
    v[2 * i + 1] = bf2f((uint16_t)(w[i] >> 16));
  }
}
__device__ __forceinline__ void ld8f(const float* p, bool ok, float v[8]) {
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  if (ok) {
    a = *reinterpret_cast<const float4*>(p);
    b = *reinterpret_cast<const float4*>(p + 4);
  }
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__device__ __forceinline__ bf16x8 pack8(const float v[8]) {
  uint4 u = make_uint4(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]), f2bf2(v[4], v[5]),
                       f2bf2(v[6], v[7]));
  return *reinterpret_cast<bf16x8*>(&u);
}

// 8 consecutive elements as an MFMA fragment; bf16 IO: the 16 bytes as loaded
__device__ __forceinline__ bf16x8 ld8(const uint16_t* p, bool ok) {
  uint4 u = make_uint4(0u, 0u, 0u, 0u);
  if (ok) u = *reinterpret_cast<const uint4*>(p);
  return *reinterpret_cast<bf16x8*>(&u);
}
__device__ __forceinline__ bf16x8 ld8(const float* p, bool ok) {
  float v[8];
  ld8f(p, ok, v);
  return pack8(v);
}

// two accumulator tiles (rows 0..15 and 16..31 of a 32-row k-step) as the B
// fragment of that k-step, in the perm(g, j) order
__device__ __forceinline__ bf16x8 acc_pair_frag(const float lo[4], const float hi[4]) {
  uint4 u = make_uint4(f2bf2(lo[0], lo[1]), f2bf2(lo[2], lo[3]), f2bf2(hi[0], hi[1]),
                       f2bf2(hi[2], hi[3]));
  return *reinterpret_cast<bf16x8*>(&u);
}

// One transposed read: `p` is this lane's address of 4 consecutive elements of
// its block row (row lane_c >> 2, columns 4 (lane_c & 3) ..); the lane gets
// column lane_c of the block's 4 rows.
__device__ __forceinline__ s16x4 lds_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(p));
}

// A (or B) fragment of one k-step from a row-major image with `stride` bytes per
// row: rows r0 + hi_step * jj + 4 * (this lane's share) of columns col0 .. + 15
__device__ __forceinline__ bf16x8 lds_tr_frag(const char* img, int stride, int row_lo,
                                              int row_hi, int col0, int lane) {
  const int c = lane & 15;
  const int in_blk = (c >> 2) * stride + (col0 + 4 * (c & 3)) * 2;
  s16x4 a = lds_tr(img + row_lo * stride + in_blk);
  s16x4 b = lds_tr(img + row_hi * stride + in_blk);
  s16x8 r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return *reinterpret_cast<bf16x8*>(&r);
}

template <typename T, int DH>
__global__ __launch_bounds__(A_THREADS) void mha_tile_fwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    T* __restrict__ o, float* __restrict__ lse, MhaStrides qs, MhaStrides os,
    int64_t BH, int n_heads, int T_len, float scale) {
  constexpr int KS = (DH + 31) / 32;   // k-steps over d in the score product
  constexpr int DT = DH / 16;          // 16-wide d tiles of the output
  constexpr int CH = DH / 8;           // 16-byte pieces per row
  constexpr int ROWB = DH * 2;         // image row, bytes
  __shared__ __attribute__((aligned(16))) char lds[A_WAVES][TILE_T * ROWB];

  const int wv = threadIdx.x / DR_WAVE;
  const int lane = threadIdx.x % DR_WAVE;
  const int64_t bh = (int64_t)blockIdx.x * A_WAVES + wv;
  if (bh >= BH) return;                // wave-uniform
  char* v_img = lds[wv];

  const int64_t in_off = (bh / n_heads) * qs.sb + (bh % n_heads) * qs.sh;
  const T* qb = q + in_off;
  const T* kb = k + in_off;
  const T* vb = v + in_off;
  T* ob = o + (bh / n_heads) * os.sb + (bh % n_heads) * os.sh;
  const int c = lane & 15, g = lane >> 4;

  // ---- q / k fragments straight from global, V into its row-major image ----
  bf16x8 qf[4][KS], kf[4][KS];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int row = 16 * i + c, d0 = 32 * ks + 8 * g;
      const bool ok = row < T_len && d0 < DH;
      qf[i][ks] = ld8(qb + (int64_t)row * qs.st + d0, ok);
      kf[i][ks] = ld8(kb + (int64_t)row * qs.st + d0, ok);
    }
#pragma unroll
  for (int it = 0; it < CH; ++it) {
    const int id = it * DR_WAVE + lane;
    const int row = id / CH, ch = id % CH;
    *reinterpret_cast<bf16x8*>(v_img + row * ROWB + ch * 16) =
        ld8(vb + (int64_t)row * qs.st + ch * 8, row < T_len);
  }
  wave_lds_fence();

  // ---- S^T[key][q]: rows = keys (16 ki + 4g + r), lane column = q ----
  float p[4][4][4];                    // [qi][ki][r]
#pragma unroll
  for (int qi = 0; qi < 4; ++qi)
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ki][ks], qf[qi][ks], a, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        p[qi][ki][r] = (16 * ki + 4 * g + r < T_len) ? a[r] * scale : -1e30f;
    }

  // ---- softmax of each query column: once, over all keys ----
  float m[4], l[4];
  bf16x8 pf[2][4];                     // [k-step over keys][qi]
#pragma unroll
  for (int qi = 0; qi < 4; ++qi) {
    float mx = -1e30f;
#pragma unroll
    for (int ki = 0; ki < 4; ++ki)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, p[qi][ki][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, DR_WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, DR_WAVE));
    float sum = 0.f;
#pragma unroll
    for (int ki = 0; ki < 4; ++ki)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[qi][ki][r] = __expf(p[qi][ki][r] - mx);
        sum += p[qi][ki][r];
      }
    sum += __shfl_xor(sum, 16, DR_WAVE);
    sum += __shfl_xor(sum, 32, DR_WAVE);
    m[qi] = mx;
    l[qi] = sum;
    pf[0][qi] = acc_pair_frag(p[qi][0], p[qi][1]);
    pf[1][qi] = acc_pair_frag(p[qi][2], p[qi][3]);
  }

  // ---- O^T[d][q] = V^T P^T: rows = d (16 dt + 4g + r), lane column = q ----
  f32x4 o_acc[DT][4];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) o_acc[dt][qi] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 vt = lds_tr_frag(v_img, ROWB, 32 * s + 4 * g, 32 * s + 16 + 4 * g,
                                    16 * dt, lane);
#pragma unroll
      for (int qi = 0; qi < 4; ++qi)
        o_acc[dt][qi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vt, pf[s][qi],
                                                                o_acc[dt][qi], 0, 0, 0);
    }
  }

  // ---- store: 4 consecutive d of one (t, head) row per lane ----
#pragma unroll
  for (int qi = 0; qi < 4; ++qi) {
    const int row = 16 * qi + c;
    if (row >= T_len) continue;
    const float inv_l = 1.f / l[qi];   // l >= 1: the row maximum contributes 1
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const float out[4] = {o_acc[dt][qi][0] * inv_l, o_acc[dt][qi][1] * inv_l,
                            o_acc[dt][qi][2] * inv_l, o_acc[dt][qi][3] * inv_l};
      st4(ob + (int64_t)row * os.st + 16 * dt + 4 * g, out);
    }
    if (g == 0) lse[bh * T_len + row] = m[qi] + __logf(l[qi]);
  }
}

// Backward of the whole-head tile.  Scores are queries-on-rows here
// (S[q][key], lane column = key), so P and dS feed dV^T = dO^T P and
// dK^T = Q^T dS from their accumulators; dQ^T = K^T dS^T sums over the lane
// index and takes dS through one LDS image ([key][q], 8-byte stores, transposed
// reads).  Nothing is accumulated across waves: no atomics, dq in the IO dtype.
// LDS per wave: phase 1 the Q and dO images, phase 2 (over them) the K and
// dS^T images; all four are written from the fragments already in registers.
template <int DH>
struct TileBwdLds {
  static constexpr int IMG = TILE_T * DH * 2;
  static constexpr int DS = TILE_T * DS_STRIDE;
  static constexpr int BYTES = IMG + (IMG > DS ? IMG : DS);
};

template <typename T, int DH>
__global__ __launch_bounds__(A_THREADS) void mha_tile_bwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    const T* __restrict__ o, const T* __restrict__ dout,
    const float* __restrict__ lse, T* __restrict__ dq, T* __restrict__ dk,
    T* __restrict__ dv, MhaStrides qs, MhaStrides os, int64_t BH, int n_heads,
    int T_len, float scale) {
  constexpr int KS = (DH + 31) / 32;
  constexpr int DT = DH / 16;
  constexpr int ROWB = DH * 2;
  constexpr int IMG = TileBwdLds<DH>::IMG;
  __shared__ __attribute__((aligned(16))) char lds[A_WAVES][TileBwdLds<DH>::BYTES];
  __shared__ __attribute__((aligned(16))) float stat[A_WAVES][2 * TILE_T];

  const int wv = threadIdx.x / DR_WAVE;
  const int lane = threadIdx.x % DR_WAVE;
  const int64_t bh = (int64_t)blockIdx.x * A_WAVES + wv;
  if (bh >= BH) return;                // wave-uniform
  char* img0 = lds[wv];                // Q image, then K image
  char* img1 = lds[wv] + IMG;          // dO image, then dS^T image
  float* lse_s = stat[wv];
  float* drow_s = stat[wv] + TILE_T;

  const int64_t bb = bh / n_heads, hh = bh % n_heads;
  const int64_t in_off = bb * qs.sb + hh * qs.sh;
  const int64_t o_off = bb * os.sb + hh * os.sh;
  const T* qb = q + in_off;
  const T* kb = k + in_off;
  const T* vb = v + in_off;
  const T* ob = o + o_off;
  const T* dob = dout + o_off;
  const int c = lane & 15, g = lane >> 4;

  // ---- fragments from global; Drow = rowsum(dO * O) from the same loads ----
  bf16x8 qf[4][KS], kf[4][KS], vf[4][KS], dof[4][KS];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float dsum = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int row = 16 * i + c, d0 = 32 * ks + 8 * g;
      const bool ok = row < T_len && d0 < DH;
      qf[i][ks] = ld8(qb + (int64_t)row * qs.st + d0, ok);
      kf[i][ks] = ld8(kb + (int64_t)row * qs.st + d0, ok);
      vf[i][ks] = ld8(vb + (int64_t)row * qs.st + d0, ok);
      float a[8], b[8];
      ld8f(dob + (int64_t)row * os.st + d0, ok, a);
      ld8f(ob + (int64_t)row * os.st + d0, ok, b);
#pragma unroll
      for (int e = 0; e < 8; ++e) dsum += a[e] * b[e];
      dof[i][ks] = pack8(a);
      if (d0 < DH) {
        *reinterpret_cast<bf16x8*>(img0 + row * ROWB + d0 * 2) = qf[i][ks];
        *reinterpret_cast<bf16x8*>(img1 + row * ROWB + d0 * 2) = dof[i][ks];
      }
    }
    // the 4 lanes of a row hold its DH / 8 pieces
    dsum += __shfl_xor(dsum, 16, DR_WAVE);
    dsum += __shfl_xor(dsum, 32, DR_WAVE);
    if (g == 0) drow_s[16 * i + c] = dsum;
  }
  lse_s[lane] = lane < T_len ? lse[bh * T_len + lane] : 0.f;
  wave_lds_fence();

  // ---- P and dS, [q][key]: rows = q (16 qi + 4g + r), lane column = key ----
  bf16x8 pf[2][4], dsf[2][4];          // [k-step over q][ki]
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
      float pp[2][4], dd[2][4];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int qi = 2 * s + half;
        f32x4 sa = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[qi][ks], kf[ki][ks], sa, 0, 0, 0);
          da = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dof[qi][ks], vf[ki][ks], da, 0, 0, 0);
        }
        const float4 l4 = *reinterpret_cast<const float4*>(lse_s + 16 * qi + 4 * g);
        const float4 r4 = *reinterpret_cast<const float4*>(drow_s + 16 * qi + 4 * g);
        const float lv[4] = {l4.x, l4.y, l4.z, l4.w};
        const float rv[4] = {r4.x, r4.y, r4.z, r4.w};
        const bool kok = 16 * ki + c < T_len;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = kok && (16 * qi + 4 * g + r < T_len);
          const float pv = ok ? __expf(sa[r] * scale - lv[r]) : 0.f;
          pp[half][r] = pv;
          dd[half][r] = ok ? pv * (da[r] - rv[r]) * scale : 0.f;
        }
      }
      pf[s][ki] = acc_pair_frag(pp[0], pp[1]);
      dsf[s][ki] = acc_pair_frag(dd[0], dd[1]);
    }

  // ---- dV^T = dO^T P, dK^T = Q^T dS: rows = d, lane column = key ----
  T* dkb = dk + in_off;
  T* dvb = dv + in_off;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    f32x4 dv_acc[4], dk_acc[4];
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
      dv_acc[ki] = f32x4{0.f, 0.f, 0.f, 0.f};
      dk_acc[ki] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 dot = lds_tr_frag(img1, ROWB, 32 * s + 4 * g, 32 * s + 16 + 4 * g,
                                     16 * dt, lane);
      const bf16x8 qt = lds_tr_frag(img0, ROWB, 32 * s + 4 * g, 32 * s + 16 + 4 * g,
                                    16 * dt, lane);
#pragma unroll
      for (int ki = 0; ki < 4; ++ki) {
        dv_acc[ki] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dot, pf[s][ki], dv_acc[ki], 0, 0, 0);
        dk_acc[ki] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qt, dsf[s][ki], dk_acc[ki], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
      const int row = 16 * ki + c;
      if (row >= T_len) continue;
      const float a[4] = {dv_acc[ki][0], dv_acc[ki][1], dv_acc[ki][2], dv_acc[ki][3]};
      const float b[4] = {dk_acc[ki][0], dk_acc[ki][1], dk_acc[ki][2], dk_acc[ki][3]};
      st4(dvb + (int64_t)row * qs.st + 16 * dt + 4 * g, a);
      st4(dkb + (int64_t)row * qs.st + 16 * dt + 4 * g, b);
    }
  }

  // ---- phase 2 images over phase 1's: K [key][d], dS^T [key][q] ----
  wave_lds_fence();                    // the Q / dO image reads are done
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = 32 * ks + 8 * g;
      if (d0 < DH)
        *reinterpret_cast<bf16x8*>(img0 + (16 * i + c) * ROWB + d0 * 2) = kf[i][ks];
    }
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
      // rows q = 32 s + 4g .. + 3 and 32 s + 16 + 4g .. + 3 of key column 16 ki + c
      const uint4 u = *reinterpret_cast<const uint4*>(&dsf[s][ki]);
      char* dst = img1 + (16 * ki + c) * DS_STRIDE + (32 * s + 4 * g) * 2;
      *reinterpret_cast<uint2*>(dst) = make_uint2(u.x, u.y);
      *reinterpret_cast<uint2*>(dst + 32) = make_uint2(u.z, u.w);
    }
  wave_lds_fence();

  // ---- dQ^T = K^T dS^T: rows = d, lane column = q; natural key order ----
  T* dqb = dq + in_off;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    f32x4 dq_acc[4];
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) dq_acc[qi] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 kt = lds_tr_frag(img0, ROWB, 32 * s + 8 * g, 32 * s + 8 * g + 4,
                                    16 * dt, lane);
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        const bf16x8 dst = lds_tr_frag(img1, DS_STRIDE, 32 * s + 8 * g,
                                       32 * s + 8 * g + 4, 16 * qi, lane);
        dq_acc[qi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kt, dst, dq_acc[qi], 0, 0, 0);
      }
    }
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
      const int row = 16 * qi + c;
      if (row >= T_len) continue;
      const float a[4] = {dq_acc[qi][0], dq_acc[qi][1], dq_acc[qi][2], dq_acc[qi][3]};
      st4(dqb + (int64_t)row * qs.st + 16 * dt + 4 * g, a);
    }
  }
}

// The one place that chooses the kernels: the whole-head tile bodies where all
// keys and queries of a head fit one wave, the flash-style bodies otherwise
// (and always with per-sample lengths).
static bool mha_whole_tile(int T_len, int D) {
  return T_len >= 1 && T_len <= TILE_T && (D == 16 || D == 32 || D == 64);
}

// run f with the head dim of the whole-head tile kernels as a tag
template <typename F>
static hipError_t with_tile_dh(int D, F&& f) {
  if (D == 16) return f(std::integral_constant<int, 16>{});
  if (D == 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

template <typename T>
static hipError_t mha_fwd_launch(const void* q, const void* k, const void* v,
                                 void* o, float* lse, int64_t B, int n_heads,
                                 int T_len, int D, float scale, const int* kv_len,
                                 MhaStrides qs, MhaStrides os, hipStream_t stream) {
  const int64_t BH = B * n_heads;
  if (kv_len == nullptr && mha_whole_tile(T_len, D)) {
    dim3 grid((unsigned)((BH + A_WAVES - 1) / A_WAVES));
    return with_tile_dh(D, [&](auto dh) {
      hipLaunchKernelGGL((mha_tile_fwd_kernel<T, decltype(dh)::value>), grid,
                         dim3(A_THREADS), 0, stream, (const T*)q, (const T*)k,
                         (const T*)v, (T*)o, lse, qs, os, BH, n_heads, T_len,
                         scale);
      return hipGetLastError();
    });
  }
  dim3 grid((T_len + QT - 1) / QT, (unsigned)BH);
  auto flash = [&](auto varlen) {
    hipLaunchKernelGGL((mha_fwd_kernel<T, decltype(varlen)::value>), grid,
                       dim3(A_THREADS), 0, stream, (const T*)q, (const T*)k,
                       (const T*)v, (T*)o, lse, qs, os, T_len, D, scale, kv_len,
                       n_heads);
    return hipGetLastError();
  };
  return kv_len != nullptr ? flash(std::true_type{}) : flash(std::false_type{});
}

template <typename T>
static hipError_t mha_bwd_launch(const void* q, const void* k, const void* v,
                                 const void* o, const void* dout, const float* lse,
                                 void* dq, void* dk, void* dv, int64_t B,
                                 int n_heads, int T_len, int D, float scale,
                                 MhaStrides qs, MhaStrides os, MhaStrides dqs,
                                 hipStream_t stream) {
  const int64_t BH = B * n_heads;
  if (mha_whole_tile(T_len, D)) {
    dim3 grid((unsigned)((BH + A_WAVES - 1) / A_WAVES));
    return with_tile_dh(D, [&](auto dh) {
      hipLaunchKernelGGL((mha_tile_bwd_kernel<T, decltype(dh)::value>), grid,
                         dim3(A_THREADS), 0, stream, (const T*)q, (const T*)k,
                         (const T*)v, (const T*)o, (const T*)dout, lse, (T*)dq,
                         (T*)dk, (T*)dv, qs, os, BH, n_heads, T_len, scale);
      return hipGetLastError();
    });
  }
  dim3 grid((T_len + 63) / 64, (unsigned)BH);
  hipLaunchKernelGGL((mha_bwd_kernel<T>), grid, dim3(A_THREADS), 0, stream,
                     (const T*)q, (const T*)k, (const T*)v, (const T*)o,
                     (const T*)dout, lse, (float*)dq, (T*)dk, (T*)dv, qs, os, dqs,
                     T_len, D, scale, n_heads);
  return hipGetLastError();
}

static MhaStrides mha_strides(const int64_t* s) { return MhaStrides{s[0], s[1], s[2]}; }

}  // namespace dr

// Entry contracts: kernels.h.
extern "C" {

int dr_mha_bwd_writes_dq(int T_len, int D) { return dr::mha_whole_tile(T_len, D) ? 1 : 0; }

int dr_mha_bwd(const void* q, const void* k, const void* v, const void* o,
               const void* dout, const float* lse, void* dq, void* dk, void* dv,
               int64_t B, int n_heads, int T_len, int D, float scale, int is_bf16,
               const int64_t* qkv_strides, const int64_t* o_strides,
               const int64_t* dq_strides, hipStream_t stream) {
  return (int)dr::with_io_type(is_bf16, [&](auto io) {
    return dr::mha_bwd_launch<typename decltype(io)::type>(
        q, k, v, o, dout, lse, dq, dk, dv, B, n_heads, T_len, D, scale,
        dr::mha_strides(qkv_strides), dr::mha_strides(o_strides),
        dr::mha_strides(dq_strides), stream);
  });
}

int dr_mha_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
               int64_t B, int n_heads, int T_len, int D, float scale, int is_bf16,
               const int* kv_len, const int64_t* qkv_strides,
               const int64_t* o_strides, hipStream_t stream) {
  return (int)dr::with_io_type(is_bf16, [&](auto io) {
    return dr::mha_fwd_launch<typename decltype(io)::type>(
        q, k, v, o, lse, B, n_heads, T_len, D, scale, kv_len,
        dr::mha_strides(qkv_strides), dr::mha_strides(o_strides), stream);
  });
}

}  // extern "C"
