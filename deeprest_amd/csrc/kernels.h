// The C ABI of the deeprest_amd kernels: the one place an entry is declared.
// bindings.cpp calls through these declarations and every .hip file includes
// them, so a definition that disagrees with its declaration does not compile.
//
// Status convention: an entry that launches anything returns the hipError_t of
// its set-up or of its first failing launch as an int, 0 on success; no launch
// follows a failed one.  The value must be used (bindings.cpp: launch_check).
// The entries validate nothing about their pointers: every operand is checked
// by the binding before the call.  All pointers are device memory and all
// launches go to `stream`.  `is_bf16`: the IO element type, bf16 (non-zero) or
// f32; `void*` operands are of that type unless said otherwise.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

extern "C" {

// ------------------------------------------ dropout + residual + layer norm
// has_mask: seed != nullptr; has_norm: w != nullptr.  branch == nullptr
// (forward) / d_r_out == nullptr (backward) is plain LayerNorm, which takes
// no seed and needs w.  Operands a mode does not use are null.  n_rows > 0.
// seed: the (key, stream) pair; keep iff the Philox word >= thr.
[[nodiscard]] int dr_dropout_add_ln_fwd(
    const void* branch, const void* residual, const float* w, const float* b,
    const int64_t* seed, uint32_t thr, float scale, void* r_out, void* normed,
    float* mean, float* rstd, int64_t n_rows, int D, float eps, int is_bf16,
    hipStream_t stream);
// At least one of seed / w is non-null: without either, d_branch and
// d_residual are both d_r_out, nothing is launched and 0 comes back.
// dwdb_part: (n_blocks, 2, D) f32 dw / db partials, zeroed by the caller;
// n_blocks is the grid.  With w, 2 * D floats of dynamic LDS per block.
[[nodiscard]] int dr_dropout_add_ln_bwd(
    const void* d_normed, const void* d_r_out, const void* r_out,
    const float* w, const float* mean, const float* rstd, const int64_t* seed,
    uint32_t thr, float scale, void* d_res, void* d_branch, float* dwdb_part,
    int n_blocks, int64_t n_rows, int D, int is_bf16, hipStream_t stream);

// ------------------------------------------------------------------ pinball
// out (N, Q), labels (N,), quantiles (Q,), Q <= 8.  loss: one f32, zeroed by
// the caller (the blocks add into it).  N == 0 is a valid launch.
[[nodiscard]] int dr_pinball_fwd(
    const void* out, const float* labels, const float* quantiles, int Q,
    int64_t N, float inv_count, float* loss, int is_bf16, hipStream_t stream);
// grad_loss: the upstream gradient, one f32 read on the device.
[[nodiscard]] int dr_pinball_bwd(
    const void* out, const float* labels, const float* quantiles, int Q,
    int64_t N, const float* grad_loss, float inv_n, void* dout, int is_bf16,
    hipStream_t stream);
// Copies of the (M,) workspaces that the masked forward spreads its flushes
// over: 16 while one column tile holds every metric (M <= 256: all ~2048
// blocks would add into the same M addresses), 1 above (the tiles already
// spread them and the finalize block would have 16x to read).
int dr_pinball_masked_slots(int M);
// out (R, M, Q), labels (R, M); R > 0, M > 0.  wsum / wcnt: (slots, M) each,
// zeroed by the caller.  The second (finalize) launch writes loss and every
// w[m], the per-metric gradient weights the backward reads.
[[nodiscard]] int dr_pinball_masked_fwd(
    const void* out, const float* labels, const float* quantiles, int Q,
    int64_t R, int M, float* wsum, int* wcnt, float* loss, float* w,
    int is_bf16, hipStream_t stream);
[[nodiscard]] int dr_pinball_masked_bwd(
    const void* out, const float* labels, const float* quantiles, int Q,
    int64_t R, int M, const float* grad_loss, const float* w, void* dout,
    int is_bf16, hipStream_t stream);

// --------------------------------------------------------------- fused adam
// meta: 6 * nt int64 entries, [p, g, m, v pointers] x nt, the cumulative end
// offsets and one step entry per tensor (adam.hip); total = the last offset.
// step: the step the by-value bias factors are computed for; a thread
// recomputes them only where a tensor's own step differs.
[[nodiscard]] int dr_fused_adam(
    const int64_t* meta, int nt, int64_t total, float lr, float beta1,
    float beta2, float eps, float weight_decay, int64_t step,
    hipStream_t stream);
// Step counter and learning rate in device memory (graph-capturable); the
// table's step column holds each tensor's lag behind *step_ptr.
[[nodiscard]] int dr_fused_adam_dev(
    const int64_t* meta, int nt, int64_t total, const float* lr_ptr,
    float beta1, float beta2, float eps, float weight_decay,
    const int* step_ptr, hipStream_t stream);

// ---------------------------------------------------------------------- gru
// H = 128.  xg (B, TT, 3H), gamma / beta (C, 3H), w_hh (3H, H) bf16 whatever
// the IO type, b_hh (3H,) f32, h0 (B, C, H).  B == 0 is an error.
//
// 1 when a saving forward at (B, C) runs the quantile-head projection inside
// the kernel (dr_gru_fwd then takes wh_fwd / out / O), 0 when the caller does
// the projection itself.
int dr_gru_fwd_fuses_heads(int B, int C);
// Bytes of the operand-image buffer that dr_gru_fwd, dr_gru_decode and
// dr_gru_bwd take as `images`: device memory, 16-byte aligned, contents
// undefined on entry.  The entries build the pi-ordered gamma / beta / b_hh
// images in it, on the stream, where the variant they pick streams its FiLM
// operands (gamma / beta / b_hh themselves stay natural-layout).
int64_t dr_gru_operand_images_bytes(int C, int is_bf16);
// h_all (B, TT, C, H); saves (B, TT, C, 2H) with save, else null.
// wh_fwd != nullptr (save only, where dr_gru_fwd_fuses_heads says so): the
// (32, H) bf16 head weight image of dr_gru_decode; the kernel also writes
// out (B, TT, C, O).  Otherwise wh_fwd / out are null and O is 0.
[[nodiscard]] int dr_gru_fwd(
    const void* xg, const void* gamma, const void* beta, const void* w_hh,
    const float* b_hh, const void* h0, void* h_all, void* saves,
    const void* wh_fwd, void* out, int O, int B, int TT, int C, int reverse,
    int save, int fp8, int is_bf16, void* images, hipStream_t stream);
// Inference decode: GRU sequence + head projection, no h_all.  wh_fwd is the
// (32, H) bf16 head weight image, rows >= O exact zero; out (B, TT, C, O),
// h_last (B, C, H).  lens == nullptr: every row runs all TT steps; otherwise
// (B,) int32 per-sample lengths (clamped to [1, TT] by the kernel) and out
// must arrive zeroed.
[[nodiscard]] int dr_gru_decode(
    const void* xg, const void* gamma, const void* beta, const void* w_hh,
    const float* b_hh, const void* h0, const void* wh_fwd, void* out,
    void* h_last, int B, int TT, int C, int O, int reverse, int fp8,
    int is_bf16, const int* lens, void* images, hipStream_t stream);
// wh_img == nullptr: grad is grad_h (B, TT, C, H), the unfused path.
// Otherwise grad is the heads' grad_part (B, TT, C, O) and wh_img the (H, 32)
// bf16 zero-padded transposed head weight image.  w_img: (H, 3H) bf16
// pi-permuted W; w_fwd: (3H, H) bf16; dpre (B, TT, C, 4H); dh0 (B, C, H) f32.
[[nodiscard]] int dr_gru_bwd(
    const void* grad, const void* wh_img, int O, const void* w_img,
    const void* w_fwd, const void* xg, const void* gamma, const void* beta,
    const float* b_hh, const void* h0, const void* h_all, const void* saves,
    void* dpre, float* dh0, int B, int TT, int C, int reverse, int is_bf16,
    void* images, hipStream_t stream);
// largest C the single-pass reduce kernel covers
int dr_gru_reduce_fused_max_c();
// dpre (BT, C, 4H) -> dxg (BT, 3H), dgamma (C, 3H) f32 and dbeta (C, 4H) f32,
// both zeroed by the caller; gamma_pi / xg_pi: staging images shaped like
// gamma / xg.  BT > 0, C > 0.  mode: 0 auto (single pass up to its C limit,
// the two-kernel form above it), 1 the two-kernel form, 2 the single pass (an
// error above its limit).
[[nodiscard]] int dr_gru_bwd_reduce(
    const void* dpre, const void* gamma, const void* xg, void* dxg,
    float* dgamma, float* dbeta, void* gamma_pi, void* xg_pi, int64_t BT, int C,
    int mode, int is_bf16, hipStream_t stream);

// ---------------------------------------------------------------- attention
// *_strides: {batch, head, time} element strides of a (batch, head, time, d)
// operand, d stride 1 (host memory, read before the entry returns).  q, k, v,
// dk, dv (and a dq written in the IO dtype) share qkv_strides; o and dout
// share o_strides.  lse (B, n_heads, T_len) f32.  B, n_heads, T_len >= 1;
// 8 <= D <= 64, D % 8 == 0.
//
// 1: dr_mha_bwd at these sizes writes dq itself, in the IO dtype and with the
// q strides (no atomics); 0: it accumulates into a zeroed fp32 dq with the
// strides dq_strides.
int dr_mha_bwd_writes_dq(int T_len, int D);
// kv_len == nullptr: every sample is T_len long (the training kernels).
// Otherwise (B,) int32 per-sample lengths, clamped to [1, T_len] by the kernel.
[[nodiscard]] int dr_mha_fwd(
    const void* q, const void* k, const void* v, void* o, float* lse, int64_t B,
    int n_heads, int T_len, int D, float scale, int is_bf16, const int* kv_len,
    const int64_t* qkv_strides, const int64_t* o_strides, hipStream_t stream);
[[nodiscard]] int dr_mha_bwd(
    const void* q, const void* k, const void* v, const void* o,
    const void* dout, const float* lse, void* dq, void* dk, void* dv, int64_t B,
    int n_heads, int T_len, int D, float scale, int is_bf16,
    const int64_t* qkv_strides, const int64_t* o_strides,
    const int64_t* dq_strides, hipStream_t stream);

// ------------------------------------------------------------------- sanity
// out (N, TT, M, 3); measured, scores, flags (N, TT, M); y_min, y_scale (M,);
// max_score, n_flagged, first_flag, n_observed (N, M).  base (N, TT, M),
// conformal (M,), lengths (N,) and bands (N, TT, M, 3) may be null.
// N * M > 0, TT > 0, min_run >= 1.
[[nodiscard]] int dr_sanity_scores(
    const void* out, const float* measured, const float* base,
    const float* y_min, const float* y_scale, const float* conformal,
    const int* lengths, int64_t N, int TT, int M, int log1p, float threshold,
    int min_run, float* scores, uint8_t* flags, float* max_score,
    int* n_flagged, int* first_flag, int* n_observed, float* bands, int is_bf16,
    hipStream_t stream);

}  // extern "C"
