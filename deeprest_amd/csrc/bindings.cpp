// Python bindings for the deeprest_amd CDNA4 kernels (torch extension).
//
// Tensor checking / allocation / stream plumbing lives here; the kernels in
// *.hip are torch-free and exposed through a C ABI (kernels.h).  No tensor's
// data_ptr reaches an entry before it has been checked for device, dtype,
// contiguity and the element count the kernel will index: a bad operand is an
// exception before any launch, a refused launch an exception after it.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "kernels.h"

namespace {

bool is_bf16(const at::Tensor& t) { return t.scalar_type() == at::kBFloat16; }

void check_dtype(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kFloat,
              name, " must be bf16 or f32, got ", t.scalar_type());
}

hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

// a kernel entry's return value: a rejected set-up or launch is the caller's
// error, never a silently wrong result
void launch_check(int err, const char* entry) {
  TORCH_CHECK(err == 0, entry, " failed (HIP error ", err, ": ",
              hipGetErrorString((hipError_t)err), ")");
}

// operand `t`: on ref's GPU, of dtype dt, contiguous, with numel elements
void check_operand(const at::Tensor& t, const char* name, const at::Tensor& ref,
                   at::ScalarType dt, int64_t numel) {
  TORCH_CHECK(ref.is_cuda() && t.device() == ref.device(), name,
              " must be on the GPU of the call's first operand (", ref.device(),
              "), got ", t.device());
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.numel() == numel, name, " must have ", numel, " elements, got ",
              t.numel());
}

// same, with exactly this shape
void check_operand(const at::Tensor& t, const char* name, const at::Tensor& ref,
                   at::ScalarType dt, at::IntArrayRef shape) {
  TORCH_CHECK(t.sizes() == shape, name, " must have shape ", shape, ", got ",
              t.sizes());
  check_operand(t, name, ref, dt, t.numel());
}

// optional per-sample lengths of the inference kernels: (B,) int32 on the
// input's device.  The VALUES are not checked (no host sync): the kernels
// clamp each one to [1, T] themselves.
const int* lengths_ptr(const c10::optional<at::Tensor>& lengths,
                       const at::Tensor& like, int64_t B, const char* name) {
  if (!lengths.has_value()) return nullptr;
  const at::Tensor& l = *lengths;
  TORCH_CHECK(l.scalar_type() == at::kInt, name, " must be int32, got ",
              l.scalar_type());
  TORCH_CHECK(l.is_cuda() && l.device() == like.device(), name,
              " must be on the input's device");
  TORCH_CHECK(l.is_contiguous() && l.numel() == B, name,
              " must be contiguous with one entry per batch sample (", B,
              "), got ", l.numel());
  return l.data_ptr<int>();
}

// ------------------------------------------- dropout + residual + layer norm
// seed absent: no mask (p == 0 or eval).  w/b absent: plain dropout_add.
struct DropoutArgs {
  const int64_t* seed = nullptr;
  uint32_t thr = 0;
  float scale = 1.f;
};

DropoutArgs dropout_args(const c10::optional<at::Tensor>& seed, double p,
                         const at::Tensor& like) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0, 1), got ", p);
  DropoutArgs a;
  if (!seed.has_value()) return a;
  const at::Tensor& s = *seed;
  TORCH_CHECK(p > 0.0, "a dropout seed was given with p == 0");
  TORCH_CHECK(s.is_cuda() && s.device() == like.device() &&
                  s.scalar_type() == at::kLong && s.numel() == 2 &&
                  s.is_contiguous(),
              "dropout seed must be a contiguous int64 (key, stream) pair on ",
              like.device());
  a.seed = s.data_ptr<int64_t>();
  // keep iff word >= thr, thr = min(floor(p * 2^32), 2^32 - 1), in double
  a.thr = (uint32_t)std::min(std::floor(p * 4294967296.0), 4294967295.0);
  a.scale = (float)(1.0 / (1.0 - p));
  return a;
}

// branch absent: plain layer_norm(residual); needs w/b, takes no seed, and
// returns an empty r_out (the row is not copied).
std::vector<at::Tensor> dropout_add_ln_forward(c10::optional<at::Tensor> branch,
                                               at::Tensor residual,
                                               c10::optional<at::Tensor> w,
                                               c10::optional<at::Tensor> b,
                                               c10::optional<at::Tensor> seed,
                                               double p, double eps) {
  const at::cuda::CUDAGuard guard(residual.device());
  check_dtype(residual, "residual");
  TORCH_CHECK(residual.is_cuda() && residual.is_contiguous());
  TORCH_CHECK(residual.dim() >= 1 && residual.size(-1) > 0);
  const bool has_add = branch.has_value(), has_norm = w.has_value();
  TORCH_CHECK(b.has_value() == has_norm, "weight and bias go together");
  if (has_add) {
    check_operand(*branch, "branch", residual, residual.scalar_type(),
                  residual.sizes());
  } else {
    TORCH_CHECK(has_norm && !seed.has_value(),
                "without a branch the op is layer_norm: weight/bias, no seed");
  }
  int D = (int)residual.size(-1);
  int64_t n_rows = residual.numel() / D;
  DropoutArgs da = dropout_args(seed, p, residual);
  auto r_out = has_add ? at::empty_like(residual) : at::empty({0}, residual.options());
  auto f32 = residual.options().dtype(at::kFloat);
  at::Tensor normed, mean, rstd;
  if (has_norm) {
    check_operand(*w, "layer_norm weight", residual, at::kFloat, D);
    check_operand(*b, "layer_norm bias", residual, at::kFloat, D);
    normed = at::empty_like(residual);
    mean = at::empty({n_rows}, f32);
    rstd = at::empty({n_rows}, f32);
  } else {
    normed = at::empty({0}, residual.options());
    mean = at::empty({0}, f32);
    rstd = at::empty({0}, f32);
  }
  if (n_rows > 0)
    launch_check(
        dr_dropout_add_ln_fwd(
            has_add ? branch->data_ptr() : nullptr, residual.data_ptr(),
            has_norm ? w->data_ptr<float>() : nullptr,
            has_norm ? b->data_ptr<float>() : nullptr, da.seed, da.thr, da.scale,
            has_add ? r_out.data_ptr() : nullptr,
            has_norm ? normed.data_ptr() : nullptr,
            has_norm ? mean.data_ptr<float>() : nullptr,
            has_norm ? rstd.data_ptr<float>() : nullptr, n_rows, D, (float)eps,
            is_bf16(residual), cur_stream()),
        "dr_dropout_add_ln_fwd");
  return {r_out, normed, mean, rstd};
}

// returns {d_residual, d_branch, dw, db}; without a mask d_branch IS
// d_residual, without a norm d_residual IS d_r_out and dw/db are empty.
// d_r_out absent: layer_norm backward, r_out is its x and d_residual its dx.
std::vector<at::Tensor> dropout_add_ln_backward(c10::optional<at::Tensor> d_normed,
                                                c10::optional<at::Tensor> d_r_out,
                                                at::Tensor r_out,
                                                c10::optional<at::Tensor> w,
                                                c10::optional<at::Tensor> mean,
                                                c10::optional<at::Tensor> rstd,
                                                c10::optional<at::Tensor> seed,
                                                double p) {
  const at::cuda::CUDAGuard guard(r_out.device());
  check_dtype(r_out, "r_out");
  TORCH_CHECK(r_out.is_cuda() && r_out.is_contiguous());
  TORCH_CHECK(r_out.dim() >= 1 && r_out.size(-1) > 0);
  const auto dt = r_out.scalar_type();
  const bool has_add = d_r_out.has_value(), has_norm = w.has_value();
  if (has_add) {
    check_operand(*d_r_out, "d_r_out", r_out, dt, r_out.sizes());
  } else {
    TORCH_CHECK(has_norm && !seed.has_value(),
                "without d_r_out the op is layer_norm: weight, no seed");
  }
  TORCH_CHECK(d_normed.has_value() == has_norm && mean.has_value() == has_norm &&
                  rstd.has_value() == has_norm,
              "d_normed, weight, mean and rstd go together");
  int D = (int)r_out.size(-1);
  int64_t n_rows = r_out.numel() / D;
  DropoutArgs da = dropout_args(seed, p, r_out);
  const bool has_mask = da.seed != nullptr;
  auto f32 = r_out.options().dtype(at::kFloat);
  if (!has_norm && !has_mask) return {*d_r_out, *d_r_out, at::empty({0}, f32), at::empty({0}, f32)};
  int n_blocks = (int)std::min<int64_t>((n_rows + 3) / 4, 1024);
  if (n_blocks == 0) n_blocks = 1;
  at::Tensor d_res, part;
  if (has_norm) {
    check_operand(*d_normed, "d_normed", r_out, dt, r_out.sizes());
    check_operand(*w, "layer_norm weight", r_out, at::kFloat, D);
    check_operand(*mean, "layer_norm mean", r_out, at::kFloat, n_rows);
    check_operand(*rstd, "layer_norm rstd", r_out, at::kFloat, n_rows);
    // dw/db partials live in 2 * D floats of dynamic LDS per block
    TORCH_CHECK(D <= 8192, "layer_norm backward supports D <= 8192, got ", D);
    d_res = at::empty_like(r_out);
    part = at::zeros({n_blocks, 2, D}, f32);
  } else {
    d_res = *d_r_out;
  }
  at::Tensor d_branch = has_mask ? at::empty_like(r_out) : d_res;
  if (n_rows > 0)
    launch_check(
        dr_dropout_add_ln_bwd(
            has_norm ? d_normed->data_ptr() : nullptr,
            has_add ? d_r_out->data_ptr() : nullptr, r_out.data_ptr(),
            has_norm ? w->data_ptr<float>() : nullptr,
            has_norm ? mean->data_ptr<float>() : nullptr,
            has_norm ? rstd->data_ptr<float>() : nullptr, da.seed, da.thr,
            da.scale, has_norm ? d_res.data_ptr() : nullptr,
            has_mask ? d_branch.data_ptr() : nullptr,
            has_norm ? part.data_ptr<float>() : nullptr, n_blocks, n_rows, D,
            is_bf16(r_out), cur_stream()),
        "dr_dropout_add_ln_bwd");
  if (!has_norm) return {d_res, d_branch, at::empty({0}, f32), at::empty({0}, f32)};
  auto sums = part.sum(0);  // (2, D)
  return {d_res, d_branch, sums[0], sums[1]};
}

// ---------------------------------------------------------------- pinball
// outputs (..., Q), labels with one entry per output row (any rank), q (Q,)
struct PinballShape {
  int Q;
  int64_t N;
};

static PinballShape pinball_checks(const at::Tensor& outputs,
                                   const at::Tensor& labels, const at::Tensor& q) {
  check_dtype(outputs, "pinball outputs");
  TORCH_CHECK(outputs.is_cuda() && outputs.is_contiguous() && outputs.dim() >= 1,
              "pinball outputs must be a contiguous (..., Q) GPU tensor");
  PinballShape s;
  s.Q = (int)outputs.size(-1);
  TORCH_CHECK(s.Q >= 1 && s.Q <= 8, "pinball wants 1 to 8 quantiles, got ", s.Q);
  s.N = outputs.numel() / s.Q;
  check_operand(labels, "pinball labels", outputs, at::kFloat, s.N);
  check_operand(q, "pinball quantiles", outputs, at::kFloat, s.Q);
  return s;
}

at::Tensor pinball_forward(at::Tensor outputs, at::Tensor labels, at::Tensor q) {
  const at::cuda::CUDAGuard guard(outputs.device());
  const PinballShape s = pinball_checks(outputs, labels, q);
  auto loss = at::zeros({}, outputs.options().dtype(at::kFloat));
  float inv_count = s.N > 0 ? 1.0f / (float)s.N : 0.f;
  launch_check(dr_pinball_fwd(outputs.data_ptr(), labels.data_ptr<float>(),
                              q.data_ptr<float>(), s.Q, s.N, inv_count,
                              loss.data_ptr<float>(), is_bf16(outputs),
                              cur_stream()),
               "dr_pinball_fwd");
  return loss;
}

// The upstream grad stays on the device (no .item() host sync: the kernel
// reads it, so the whole loss backward is hipGraph-capturable).
at::Tensor pinball_backward(at::Tensor grad, at::Tensor outputs, at::Tensor labels,
                            at::Tensor q) {
  const at::cuda::CUDAGuard guard(outputs.device());
  const PinballShape s = pinball_checks(outputs, labels, q);
  check_operand(grad, "pinball grad", outputs, at::kFloat, 1);
  auto dout = at::empty_like(outputs);
  float inv_n = s.N > 0 ? 1.f / (float)s.N : 0.f;
  launch_check(dr_pinball_bwd(outputs.data_ptr(), labels.data_ptr<float>(),
                              q.data_ptr<float>(), s.Q, s.N,
                              grad.data_ptr<float>(), inv_n, dout.data_ptr(),
                              is_bf16(outputs), cur_stream()),
               "dr_pinball_bwd");
  return dout;
}

// Masked variant: a non-finite label is "not observed".  outputs (..., M, Q),
// labels (..., M).  Returns {loss, w}: w (M,) f32 holds each metric's gradient
// weight 1/(Mp*cnt[m]) (0 for a metric with no present label), which the
// backward reads on the device.  No host sync: the mask may change between
// replays of a captured graph.
struct MaskedShape {
  int Q, M;
  int64_t R;
};

static MaskedShape pinball_masked_checks(const at::Tensor& outputs,
                                         const at::Tensor& labels,
                                         const at::Tensor& q) {
  check_dtype(outputs, "pinball outputs");
  TORCH_CHECK(labels.scalar_type() == at::kFloat, "pinball labels must be f32");
  TORCH_CHECK(outputs.is_contiguous() && labels.is_contiguous());
  TORCH_CHECK(outputs.is_cuda() && labels.device() == outputs.device() &&
                  q.device() == outputs.device(),
              "pinball operands must all be on the outputs' GPU");
  TORCH_CHECK(outputs.dim() >= 2 && labels.dim() == outputs.dim() - 1,
              "masked pinball wants outputs (..., M, Q) and labels (..., M)");
  MaskedShape s;
  s.Q = (int)outputs.size(-1);
  TORCH_CHECK(s.Q <= 8, "at most 8 quantiles");
  TORCH_CHECK(q.scalar_type() == at::kFloat && q.is_contiguous() &&
                  q.numel() == s.Q,
              "quantiles must be a contiguous f32 tensor with one entry per output");
  TORCH_CHECK(outputs.size(-2) < (1LL << 31), "too many metrics");
  s.M = (int)outputs.size(-2);
  TORCH_CHECK(labels.size(-1) == s.M && labels.numel() * s.Q == outputs.numel(),
              "labels do not match outputs");
  s.R = s.M > 0 ? labels.numel() / s.M : 0;
  TORCH_CHECK(s.R < (1LL << 31), "per-metric counts are int32: B*T must be < 2^31");
  return s;
}

std::vector<at::Tensor> pinball_masked_forward(at::Tensor outputs, at::Tensor labels,
                                               at::Tensor q) {
  const at::cuda::CUDAGuard guard(outputs.device());
  const MaskedShape s = pinball_masked_checks(outputs, labels, q);
  auto f32 = outputs.options().dtype(at::kFloat);
  if (s.R == 0 || s.M == 0 || s.Q == 0)
    return {at::zeros({}, f32), at::zeros({s.M}, f32)};
  // the finalize launch writes the loss and every w[m]
  auto loss = at::empty({}, f32);
  auto w = at::empty({s.M}, f32);
  // [0]: per-metric fp32 sums (zero bits are 0.0f), [1]: int counts; `slots`
  // copies of each, which the finalize launch adds up
  const int64_t slots = dr_pinball_masked_slots(s.M);
  auto ws = at::zeros({2, slots, s.M}, outputs.options().dtype(at::kInt));
  int* cnt = ws.data_ptr<int>() + slots * s.M;
  launch_check(
      dr_pinball_masked_fwd(outputs.data_ptr(), labels.data_ptr<float>(),
                            q.data_ptr<float>(), s.Q, s.R, s.M,
                            reinterpret_cast<float*>(ws.data_ptr<int>()), cnt,
                            loss.data_ptr<float>(), w.data_ptr<float>(),
                            is_bf16(outputs), cur_stream()),
      "dr_pinball_masked_fwd");
  return {loss, w};
}

at::Tensor pinball_masked_backward(at::Tensor grad, at::Tensor outputs,
                                   at::Tensor labels, at::Tensor q, at::Tensor w) {
  const at::cuda::CUDAGuard guard(outputs.device());
  const MaskedShape s = pinball_masked_checks(outputs, labels, q);
  check_operand(grad, "pinball grad", outputs, at::kFloat, 1);
  TORCH_CHECK(w.scalar_type() == at::kFloat && w.is_contiguous() &&
                  w.device() == outputs.device() && w.numel() == s.M,
              "w must be the (M,) f32 weights of pinball_masked_forward");
  auto dout = at::empty_like(outputs);
  if (s.R == 0 || s.M == 0 || s.Q == 0) return dout;
  launch_check(
      dr_pinball_masked_bwd(outputs.data_ptr(), labels.data_ptr<float>(),
                            q.data_ptr<float>(), s.Q, s.R, s.M,
                            grad.data_ptr<float>(), w.data_ptr<float>(),
                            dout.data_ptr(), is_bf16(outputs), cur_stream()),
      "dr_pinball_masked_bwd");
  return dout;
}

// ------------------------------------------------------------- fused adam
void fused_adam(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
                std::vector<int64_t> steps, double lr, double beta1, double beta2,
                double eps, double weight_decay) {
  TORCH_CHECK(!params.empty());
  TORCH_CHECK(params[0].is_cuda(), "fused_adam expects device tensors");
  const at::cuda::CUDAGuard guard(params[0].device());
  int nt = (int)params.size();
  TORCH_CHECK(grads.size() == params.size() && ms.size() == params.size() &&
                  vs.size() == params.size() && steps.size() == params.size(),
              "fused_adam: params, grads, exp_avgs, exp_avg_sqs and steps differ in length");
  std::vector<int64_t> meta(6 * nt);
  int64_t total = 0;
  for (int i = 0; i < nt; ++i) {
    const at::Tensor* ops[4] = {&params[i], &grads[i], &ms[i], &vs[i]};
    static const char* names[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
    for (int o = 0; o < 4; ++o) {
      const at::Tensor& t = *ops[o];
      TORCH_CHECK(t.scalar_type() == at::kFloat, "fused_adam expects f32 ", names[o],
                  " (tensor ", i, ")");
      TORCH_CHECK(t.is_contiguous(), "fused_adam expects contiguous ", names[o],
                  " (tensor ", i, ")");
      TORCH_CHECK(t.device() == params[0].device(), "fused_adam: ", names[o],
                  " of tensor ", i, " is on another device");
      TORCH_CHECK(t.numel() == params[i].numel(), "fused_adam: ", names[o],
                  " of tensor ", i, " has ", t.numel(), " elements, param has ",
                  params[i].numel());
    }
    TORCH_CHECK(steps[i] >= 1, "fused_adam: step of tensor ", i, " must be >= 1");
    meta[i] = (int64_t)params[i].data_ptr();
    meta[nt + i] = (int64_t)grads[i].data_ptr();
    meta[2 * nt + i] = (int64_t)ms[i].data_ptr();
    meta[3 * nt + i] = (int64_t)vs[i].data_ptr();
    total += params[i].numel();
    meta[4 * nt + i] = total;  // cumulative end offsets
    meta[5 * nt + i] = steps[i];  // the tensor's own step (bias correction)
  }
  auto meta_t = at::from_blob(meta.data(), {(int64_t)meta.size()},
                              at::TensorOptions().dtype(at::kLong))
                    .to(params[0].device(), /*non_blocking=*/false);
  // bias factors for steps[0] come from the host; a thread recomputes them
  // only where a tensor's step differs
  launch_check(dr_fused_adam(meta_t.data_ptr<int64_t>(), nt, total, (float)lr,
                             (float)beta1, (float)beta2, (float)eps,
                             (float)weight_decay, steps[0], cur_stream()),
               "dr_fused_adam");
}

// hipGraph-capturable variant: the pointer table is prebuilt on device (ops/
// adam.py caches it while pointers are stable) and the step counter is a
// device int32 scalar, so a replayed graph keeps exact bias correction with
// zero host work per step.
void fused_adam_capturable(at::Tensor meta_dev, int64_t nt, int64_t total,
                           at::Tensor step_t, at::Tensor lr_t, double beta1,
                           double beta2, double eps, double weight_decay) {
  const at::cuda::CUDAGuard guard(meta_dev.device());
  TORCH_CHECK(meta_dev.is_cuda() && meta_dev.scalar_type() == at::kLong &&
              meta_dev.is_contiguous());
  TORCH_CHECK(nt >= 1 && meta_dev.numel() == 6 * nt,
              "fused_adam_capturable: table must hold 6 entries per tensor "
              "(p, g, m, v, cumulative numel, step lag)");
  check_operand(step_t, "fused_adam step counter", meta_dev, at::kInt, 1);
  check_operand(lr_t, "fused_adam lr", meta_dev, at::kFloat, 1);
  launch_check(dr_fused_adam_dev(meta_dev.data_ptr<int64_t>(), (int)nt, total,
                                 lr_t.data_ptr<float>(), (float)beta1,
                                 (float)beta2, (float)eps, (float)weight_decay,
                                 step_t.data_ptr<int>(), cur_stream()),
               "dr_fused_adam_dev");
}

// -------------------------------------------------------------------- gru
// the GEMM streams a bf16 weight image from L2 whatever the IO dtype is
static at::Tensor gru_w_gemm(const at::Tensor& w_hh) {
  return is_bf16(w_hh) ? w_hh : w_hh.to(at::kBFloat16);
}

// operand checks shared by the forward entries
static void gru_forward_checks(const at::Tensor& xg, const at::Tensor& w_hh,
                               const at::Tensor& b_hh, const at::Tensor& h0,
                               const at::Tensor& gamma, const at::Tensor& beta) {
  check_dtype(xg, "x_gates");
  for (const at::Tensor* t : {&xg, &w_hh, &b_hh, &h0, &gamma, &beta})
    TORCH_CHECK(t->is_cuda() && t->device() == xg.device(),
                "gru operands must all be on x_gates' GPU");
  TORCH_CHECK(xg.dim() == 3, "x_gates must be (B, T, 3H)");
  TORCH_CHECK(h0.dim() == 3, "h0 must be (B, C, H)");
  int C = (int)h0.size(1), H = (int)h0.size(2);
  TORCH_CHECK(H == 128, "fused GRU kernel requires hidden size 128, got ", H);
  TORCH_CHECK(C >= 3, "fused GRU kernel requires >= 3 components, got ", C);
  TORCH_CHECK(xg.size(2) == 3 * H && w_hh.size(0) == 3 * H && w_hh.size(1) == H);
  TORCH_CHECK(gamma.sizes() == at::IntArrayRef({C, 3 * H}));
  TORCH_CHECK(h0.size(0) == xg.size(0) && beta.sizes() == gamma.sizes() &&
                  b_hh.numel() == 3 * H,
              "gru operand shapes do not match x_gates (B, T, 3H)");
  TORCH_CHECK(b_hh.scalar_type() == at::kFloat, "b_hh must be f32");
  auto dt = xg.scalar_type();
  TORCH_CHECK(w_hh.scalar_type() == dt && h0.scalar_type() == dt &&
                  gamma.scalar_type() == dt && beta.scalar_type() == dt,
              "gru operand dtypes must match x_gates");
  TORCH_CHECK(xg.is_contiguous() && w_hh.is_contiguous() && h0.is_contiguous() &&
              gamma.is_contiguous() && beta.is_contiguous() && b_hh.is_contiguous());
  TORCH_CHECK(xg.numel() < (1LL << 31),
              "x_gates too large for 32-bit staging offsets");
}

// the (32, H) bf16 head weight image of the forward kernels' head phase
static void check_wh_fwd(const at::Tensor& wh_fwd, int64_t O, int H) {
  TORCH_CHECK(O >= 1 && O <= 32, "the fused head phase needs 1 <= O <= 32, got ", O);
  TORCH_CHECK(wh_fwd.scalar_type() == at::kBFloat16 &&
                  wh_fwd.sizes() == at::IntArrayRef({32, H}) &&
                  wh_fwd.is_contiguous() && wh_fwd.is_cuda(),
              "wh_fwd must be the (32, H) bf16 head weight image");
}

// Scratch for the chain kernels' pi-ordered operand images, from the torch
// allocator (stream-ordered, no host sync: graph-capturable).  The launcher
// fills it on the current stream; it lives until the call's kernels are
// queued, and the caching allocator does not hand it to another stream.
static at::Tensor gru_operand_images(const at::Tensor& gamma, int C) {
  return at::empty({dr_gru_operand_images_bytes(C, is_bf16(gamma))},
                   gamma.options().dtype(at::kByte));
}

// Whether gru_seq_forward at these sizes takes wh_fwd and runs the head
// projection inside the kernel; callers ask here, the launcher decides.
bool gru_fwd_fuses_heads(int64_t B, int64_t C, bool save) {
  return save && dr_gru_fwd_fuses_heads((int)B, (int)C) != 0;
}

// Returns {h_all, saves}.  With wh_fwd (the decode entry's head weight image)
// and O, allowed only where gru_fwd_fuses_heads says so, the kernel runs the
// head phase too and {h_all, saves, out} comes back, out (B, T, C, O) =
// h_all @ w_head^T.
std::vector<at::Tensor> gru_seq_forward(at::Tensor xg, at::Tensor w_hh,
                                        at::Tensor b_hh, at::Tensor h0,
                                        at::Tensor gamma, at::Tensor beta,
                                        bool reverse, bool save, bool fp8,
                                        c10::optional<at::Tensor> wh_fwd,
                                        int64_t O) {
  TORCH_CHECK(!(fp8 && save), "fp8 GRU path is inference-only (no saves)");
  const at::cuda::CUDAGuard guard(xg.device());
  gru_forward_checks(xg, w_hh, b_hh, h0, gamma, beta);
  int B = (int)xg.size(0), TT = (int)xg.size(1);
  int C = (int)h0.size(1), H = (int)h0.size(2);
  TORCH_CHECK((int64_t)B * TT * C < (1LL << 31),
              "gru forward: too many (b, t, c) rows for 32-bit row indices");
  const bool heads = wh_fwd.has_value();
  if (heads) {
    TORCH_CHECK(!fp8 && gru_fwd_fuses_heads(B, C, save),
                "gru forward: no in-kernel head phase at B=", B, " C=", C,
                " save=", save, " (ask gru_fwd_fuses_heads first)");
    check_wh_fwd(*wh_fwd, O, H);
    TORCH_CHECK((int64_t)B * TT * C * O < (1LL << 31),
                "head output too large for 32-bit store offsets");
  }
  auto h_all = at::empty({B, TT, C, H}, xg.options());
  auto saves = save ? at::empty({B, TT, C, 2 * H}, xg.options())
                    : at::empty({0}, xg.options());
  auto out = heads ? at::empty({B, TT, C, O}, xg.options())
                   : at::empty({0}, xg.options());
  auto w_gemm = gru_w_gemm(w_hh);
  auto images = gru_operand_images(gamma, C);
  launch_check(
      dr_gru_fwd(xg.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                 w_gemm.data_ptr(), b_hh.data_ptr<float>(), h0.data_ptr(),
                 h_all.data_ptr(), save ? saves.data_ptr() : nullptr,
                 heads ? wh_fwd->data_ptr() : nullptr,
                 heads ? out.data_ptr() : nullptr, heads ? (int)O : 0, B, TT, C,
                 reverse ? 1 : 0, save ? 1 : 0, fp8 ? 1 : 0, is_bf16(xg),
                 images.data_ptr(), cur_stream()),
      "dr_gru_fwd");
  if (!heads) return {h_all, saves};
  return {h_all, saves, out};
}

// Inference decode: the GRU sequence with the quantile-head projection done
// per step inside the kernel; h_all is never allocated.  wh_fwd: (32, H) bf16
// with wh_fwd[o][k] = w_head[o][k] and zero rows for o >= O.  Returns
// {out (B, T, C, O), h_last (B, C, H)}.  No host sync: graph-capturable.
// lengths (optional, (B,) int32): sample b runs its own steps t < lengths[b]
// only — out is zero at the padded positions and h_last is each row's state
// after its own last valid step.
std::vector<at::Tensor> gru_seq_decode(at::Tensor xg, at::Tensor w_hh,
                                       at::Tensor b_hh, at::Tensor h0,
                                       at::Tensor gamma, at::Tensor beta,
                                       at::Tensor wh_fwd, int64_t O, bool reverse,
                                       bool fp8,
                                       c10::optional<at::Tensor> lengths) {
  const at::cuda::CUDAGuard guard(xg.device());
  gru_forward_checks(xg, w_hh, b_hh, h0, gamma, beta);
  int B = (int)xg.size(0), TT = (int)xg.size(1);
  int C = (int)h0.size(1), H = (int)h0.size(2);
  check_wh_fwd(wh_fwd, O, H);
  TORCH_CHECK((int64_t)B * TT * C * O < (1LL << 31),
              "decode output too large for 32-bit store offsets");
  const int* lens = lengths_ptr(lengths, xg, B, "gru decode lengths");
  // with lengths the kernel stores valid positions only: padding stays zero
  auto out = lens ? at::zeros({B, TT, C, O}, xg.options())
                  : at::empty({B, TT, C, O}, xg.options());
  auto h_last = at::empty({B, C, H}, xg.options());
  auto w_gemm = gru_w_gemm(w_hh);
  auto images = gru_operand_images(gamma, C);
  launch_check(
      dr_gru_decode(xg.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                    w_gemm.data_ptr(), b_hh.data_ptr<float>(), h0.data_ptr(),
                    wh_fwd.data_ptr(), out.data_ptr(), h_last.data_ptr(), B, TT,
                    C, (int)O, reverse ? 1 : 0, fp8 ? 1 : 0, is_bf16(xg), lens,
                    images.data_ptr(), cur_stream()),
      "dr_gru_decode");
  return {out, h_last};
}

// Sequential backward chain.  wh_img == nullptr: grad is grad_h (B, T, C, H).
// Otherwise grad is the quantile heads' output gradient (B, T, C, O) and the
// kernel forms grad @ w_head per step from the (H, 32) weight image.
static std::vector<at::Tensor> gru_backward_impl(
    at::Tensor grad_h, const at::Tensor* wh_img, at::Tensor w_img,
    at::Tensor w_fwd, at::Tensor xg, at::Tensor gamma, at::Tensor beta,
    at::Tensor b_hh, at::Tensor h0, at::Tensor h_all, at::Tensor saves,
    bool reverse) {
  const at::cuda::CUDAGuard guard(grad_h.device());
  check_dtype(grad_h, "gru grad");
  TORCH_CHECK(grad_h.is_cuda() && grad_h.dim() == 4 && h_all.dim() == 4,
              "gru grad and h_all must be 4-D GPU tensors");
  const auto dt = grad_h.scalar_type();
  int B = (int)h_all.size(0), TT = (int)h_all.size(1);
  int C = (int)h_all.size(2), H = (int)h_all.size(3);
  TORCH_CHECK(H == 128, "fused GRU kernel requires hidden size 128, got ", H);
  int O = 0;
  if (wh_img != nullptr) {
    O = (int)grad_h.size(3);
    TORCH_CHECK(O >= 1 && O <= 32, "fused head gradient needs 1 <= O <= 32, got ", O);
    check_operand(*wh_img, "wh_img", grad_h, at::kBFloat16, {H, 32});
  }
  check_operand(grad_h, "gru grad", grad_h, dt, {B, TT, C, wh_img ? O : H});
  check_operand(h_all, "gru h_all", grad_h, dt, {B, TT, C, H});
  // (B, T, C, 2H); empty when the forward ran without save
  check_operand(saves, "gru saves", grad_h, dt, (int64_t)B * TT * C * 2 * H);
  check_operand(xg, "x_gates", grad_h, dt, {B, TT, 3 * H});
  check_operand(h0, "h0", grad_h, dt, {B, C, H});
  check_operand(gamma, "gamma", grad_h, dt, {C, 3 * H});
  check_operand(beta, "beta", grad_h, dt, {C, 3 * H});
  check_operand(b_hh, "b_hh", grad_h, at::kFloat, 3 * H);
  // the (H, 3H) pi-permuted and the (3H, H) natural bf16 images of W_hh
  check_operand(w_img, "w_img", grad_h, at::kBFloat16, {H, 3 * H});
  check_operand(w_fwd, "w_fwd", grad_h, at::kBFloat16, {3 * H, H});
  auto dpre = at::empty({B, TT, C, 4 * H}, grad_h.options());
  auto dh0 = at::empty({B, C, H}, grad_h.options().dtype(at::kFloat));
  auto images = gru_operand_images(gamma, C);
  launch_check(
      dr_gru_bwd(grad_h.data_ptr(), wh_img ? wh_img->data_ptr() : nullptr, O,
                 w_img.data_ptr(), w_fwd.data_ptr(), xg.data_ptr(),
                 gamma.data_ptr(), beta.data_ptr(), b_hh.data_ptr<float>(),
                 h0.data_ptr(), h_all.data_ptr(), saves.data_ptr(),
                 dpre.data_ptr(), dh0.data_ptr<float>(), B, TT, C,
                 reverse ? 1 : 0, dt == at::kBFloat16, images.data_ptr(),
                 cur_stream()),
      "dr_gru_bwd");
  return {dpre, dh0};
}

std::vector<at::Tensor> gru_seq_backward_kernel(at::Tensor grad_h, at::Tensor w_img,
                                                at::Tensor w_fwd, at::Tensor xg,
                                                at::Tensor gamma, at::Tensor beta,
                                                at::Tensor b_hh, at::Tensor h0,
                                                at::Tensor h_all, at::Tensor saves,
                                                bool reverse) {
  return gru_backward_impl(grad_h, nullptr, w_img, w_fwd, xg, gamma, beta, b_hh,
                           h0, h_all, saves, reverse);
}

// grad_part: (B, T, C, O) head output gradient, O <= 32; wh_img: (H, 32) bf16
// with wh_img[n][k] = w_head[k][n] and zeros for k >= O
std::vector<at::Tensor> gru_seq_backward_heads_kernel(
    at::Tensor grad_part, at::Tensor wh_img, at::Tensor w_img, at::Tensor w_fwd,
    at::Tensor xg, at::Tensor gamma, at::Tensor beta, at::Tensor b_hh,
    at::Tensor h0, at::Tensor h_all, at::Tensor saves, bool reverse) {
  return gru_backward_impl(grad_part, &wh_img, w_img, w_fwd, xg, gamma, beta,
                           b_hh, h0, h_all, saves, reverse);
}

// reductions over dpre (B, T, C, 4H), pi-packed slices dr|dz|d_hhn|dn:
// dxg (B, T, 3H), dgamma (C, 3H) f32, and dbeta4 (C, 4H) f32 in dpre's slice
// order (its d_hhn slice is the n-part of db_hh).  mode "fused" reads every
// dpre row once (C up to gru_reduce_fused_max_c()), "split" is the two-kernel
// form that reads it twice, "auto" takes the single pass wherever it applies.
std::vector<at::Tensor> gru_bwd_reduce(at::Tensor dpre, at::Tensor gamma,
                                       at::Tensor xg, const std::string& mode) {
  const at::cuda::CUDAGuard guard(dpre.device());
  check_dtype(dpre, "dpre");
  TORCH_CHECK(dpre.is_cuda() && dpre.is_contiguous() && dpre.dim() == 4 &&
                  dpre.size(3) == 512,
              "gru_bwd_reduce: dpre must be a contiguous (B, T, C, 4H) GPU tensor");
  int64_t BT = dpre.size(0) * dpre.size(1);
  int C = (int)dpre.size(2);
  TORCH_CHECK(BT > 0 && C > 0, "gru_bwd_reduce: empty dpre");
  check_operand(gamma, "gru_bwd_reduce gamma", dpre, dpre.scalar_type(), {C, 384});
  check_operand(xg, "gru_bwd_reduce xg", dpre, dpre.scalar_type(),
                {dpre.size(0), dpre.size(1), 384});
  int mode_id = 0;
  if (mode == "split") mode_id = 1;
  else if (mode == "fused") mode_id = 2;
  else TORCH_CHECK(mode == "auto", "gru_bwd_reduce: mode must be auto, split or fused, got ", mode);
  TORCH_CHECK(mode_id != 2 || C <= dr_gru_reduce_fused_max_c(),
              "gru_bwd_reduce: the fused mode covers C <= ",
              dr_gru_reduce_fused_max_c(), ", got C = ", C);
  auto dxg = at::empty({dpre.size(0), dpre.size(1), 384}, dpre.options());
  auto dgamma = at::zeros({C, 384}, dpre.options().dtype(at::kFloat));
  auto dbeta = at::zeros({C, 512}, dpre.options().dtype(at::kFloat));
  // pi-layout staging images (see pi_permute_rows_kernel)
  auto gamma_pi = at::empty_like(gamma);
  auto xg_pi = at::empty_like(xg);
  launch_check(
      dr_gru_bwd_reduce(dpre.data_ptr(), gamma.data_ptr(), xg.data_ptr(),
                        dxg.data_ptr(), dgamma.data_ptr<float>(),
                        dbeta.data_ptr<float>(), gamma_pi.data_ptr(),
                        xg_pi.data_ptr(), BT, C, mode_id, is_bf16(dpre),
                        cur_stream()),
      "dr_gru_bwd_reduce");
  return {dxg, dgamma, dbeta};
}

// -------------------------------------------------------------------- mha
// The kernels address (batch, head, time, d) operands by element strides.
struct MhaLayout {
  int64_t s[3];
};
// (B, H, T, D) contiguous
static MhaLayout mha_bhtd(int64_t NH, int64_t T, int64_t D) {
  return {{NH * T * D, T * D, D}};
}
// one of the three parts of a packed (B, T, 3, H, D) qkv
static MhaLayout mha_packed_part(int64_t NH, int64_t T, int64_t D) {
  return {{T * 3 * NH * D, D, 3 * NH * D}};
}
// (B, T, H, D) contiguous
static MhaLayout mha_bthd(int64_t NH, int64_t T, int64_t D) {
  return {{T * NH * D, D, NH * D}};
}

static void mha_check_head_dim(int64_t D) {
  TORCH_CHECK(D >= 8 && D <= 64 && D % 8 == 0,
              "head dim must be 8..64, mult of 8, got ", D);
}

// q is a contiguous (B, H, T, D) GPU tensor; each of `like_q` matches it in
// device, dtype and shape.
static void mha_checks(
    const at::Tensor& q,
    std::initializer_list<std::pair<const at::Tensor*, const char*>> like_q) {
  check_dtype(q, "q");
  TORCH_CHECK(q.is_cuda() && q.dim() == 4 && q.is_contiguous(),
              "q must be a contiguous (B, H, T, D) GPU tensor");
  mha_check_head_dim(q.size(3));
  TORCH_CHECK(q.size(1) < (1LL << 31) && q.size(2) < (1LL << 31),
              "mha: H and T must be < 2^31");
  for (const auto& [t, name] : like_q)
    check_operand(*t, name, q, q.scalar_type(), q.sizes());
}

// kv_lengths (optional, (B,) int32): keys >= kv_lengths[b] are absent and
// rows of o / lse at or past it are zero (inference only; mha_backward does
// not know about lengths).
std::vector<at::Tensor> mha_forward(at::Tensor q, at::Tensor k, at::Tensor v,
                                    double scale,
                                    c10::optional<at::Tensor> kv_lengths) {
  const at::cuda::CUDAGuard guard(q.device());
  mha_checks(q, {{&k, "mha k"}, {&v, "mha v"}});
  int64_t B = q.size(0), NH = q.size(1);
  int T_len = (int)q.size(2), D = (int)q.size(3);
  const int* kv_len = lengths_ptr(kv_lengths, q, B, "mha kv_lengths");
  auto o = at::empty_like(q);
  auto lse = at::empty({B, NH, T_len}, q.options().dtype(at::kFloat));
  if (q.numel() == 0) return {o, lse};
  const MhaLayout l = mha_bhtd(NH, T_len, D);
  launch_check(dr_mha_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                          lse.data_ptr<float>(), B, (int)NH, T_len, D,
                          (float)scale, is_bf16(q), kv_len, l.s, l.s, cur_stream()),
               "dr_mha_fwd");
  return {o, lse};
}

// dq comes back in q's dtype where the kernel writes it itself (one key tile
// per head), as the fp32 atomic accumulator otherwise.
std::vector<at::Tensor> mha_backward(at::Tensor q, at::Tensor k, at::Tensor v,
                                     at::Tensor o, at::Tensor dout, at::Tensor lse,
                                     double scale) {
  const at::cuda::CUDAGuard guard(q.device());
  mha_checks(q, {{&k, "mha k"}, {&v, "mha v"}, {&o, "mha o"}, {&dout, "mha dout"}});
  int64_t B = q.size(0), NH = q.size(1);
  int T_len = (int)q.size(2), D = (int)q.size(3);
  check_operand(lse, "mha lse", q, at::kFloat, {B, NH, T_len});
  const bool writes_dq = dr_mha_bwd_writes_dq(T_len, D) != 0;
  auto dq = writes_dq ? at::empty_like(q)
                      : at::zeros(q.sizes(), q.options().dtype(at::kFloat));
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  if (q.numel() == 0) return {dq, dk, dv};
  const MhaLayout l = mha_bhtd(NH, T_len, D);
  launch_check(dr_mha_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                          dout.data_ptr(), lse.data_ptr<float>(), dq.data_ptr(),
                          dk.data_ptr(), dv.data_ptr(), B, (int)NH, T_len, D,
                          (float)scale, is_bf16(q), l.s, l.s, l.s, cur_stream()),
               "dr_mha_bwd");
  return {dq, dk, dv};
}

// Attention on the packed qkv GEMM output: qkv (B, T, 3*H*Dh) or
// (B, T, 3, H, Dh) contiguous -> {o (B, T, H*Dh), lse (B, H, T)}.  No copy of
// q, k, v or o is made: the kernels take the row strides and the head offset.
struct PackedShape {
  int64_t B, T, NH, D;
};

static PackedShape mha_packed_checks(const at::Tensor& qkv, int64_t n_heads) {
  check_dtype(qkv, "qkv");
  TORCH_CHECK(qkv.is_cuda(), "qkv must be a GPU tensor");
  TORCH_CHECK(qkv.is_contiguous(), "qkv must be contiguous");
  TORCH_CHECK(n_heads >= 1, "n_heads must be >= 1, got ", n_heads);
  TORCH_CHECK(qkv.dim() == 3 || qkv.dim() == 5,
              "qkv must be (B, T, 3*H*Dh) or (B, T, 3, H, Dh)");
  PackedShape s;
  s.B = qkv.size(0);
  s.T = qkv.size(1);
  s.NH = n_heads;
  if (qkv.dim() == 5) {
    TORCH_CHECK(qkv.size(2) == 3 && qkv.size(3) == n_heads,
                "qkv must be (B, T, 3, n_heads = ", n_heads, ", Dh), got ",
                qkv.sizes());
    s.D = qkv.size(4);
  } else {
    TORCH_CHECK(qkv.size(2) % (3 * n_heads) == 0,
                "qkv's last dimension (", qkv.size(2), ") is not 3 * n_heads (",
                n_heads, ") * Dh");
    s.D = qkv.size(2) / (3 * n_heads);
  }
  mha_check_head_dim(s.D);
  TORCH_CHECK(s.T >= 1 && s.T < (1LL << 31), "qkv needs 1 <= T < 2^31");
  // every (t, part, head) row starts on a 16-byte boundary (Dh % 8 == 0)
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
              "qkv must be 16-byte aligned");
  return s;
}

std::vector<at::Tensor> mha_packed_forward(at::Tensor qkv, int64_t n_heads,
                                           double scale) {
  const at::cuda::CUDAGuard guard(qkv.device());
  const PackedShape s = mha_packed_checks(qkv, n_heads);
  auto o = at::empty({s.B, s.T, s.NH * s.D}, qkv.options());
  auto lse = at::empty({s.B, s.NH, s.T}, qkv.options().dtype(at::kFloat));
  if (s.B == 0) return {o, lse};
  const int64_t part = s.NH * s.D * qkv.element_size();
  const char* base = static_cast<const char*>(qkv.data_ptr());
  const MhaLayout ql = mha_packed_part(s.NH, s.T, s.D);
  const MhaLayout ol = mha_bthd(s.NH, s.T, s.D);
  launch_check(dr_mha_fwd(base, base + part, base + 2 * part, o.data_ptr(),
                          lse.data_ptr<float>(), s.B, (int)s.NH, (int)s.T,
                          (int)s.D, (float)scale, is_bf16(qkv), nullptr, ql.s,
                          ol.s, cur_stream()),
               "dr_mha_fwd");
  return {o, lse};
}

// dout (B, T, H*Dh) contiguous -> dqkv (B, T, 3, H, Dh) in qkv's dtype, written
// by the kernel in place of its q, k, v parts.
at::Tensor mha_packed_backward(at::Tensor qkv, int64_t n_heads, at::Tensor o,
                               at::Tensor dout, at::Tensor lse, double scale) {
  const at::cuda::CUDAGuard guard(qkv.device());
  const PackedShape s = mha_packed_checks(qkv, n_heads);
  for (const at::Tensor* t : {&o, &dout})
    TORCH_CHECK(t->is_cuda() && t->device() == qkv.device() &&
                    t->scalar_type() == qkv.scalar_type() && t->is_contiguous() &&
                    t->numel() == s.B * s.T * s.NH * s.D &&
                    reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "o and dout must be contiguous (B, T, H*Dh) tensors of qkv's "
                "dtype on its device, 16-byte aligned");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
                  lse.device() == qkv.device() && lse.numel() == s.B * s.NH * s.T,
              "lse must be the (B, H, T) f32 tensor of mha_packed_forward");
  auto dqkv = at::empty({s.B, s.T, 3, s.NH, s.D}, qkv.options());
  if (s.B == 0) return dqkv;
  const int64_t part = s.NH * s.D * qkv.element_size();
  const char* base = static_cast<const char*>(qkv.data_ptr());
  char* dbase = static_cast<char*>(dqkv.data_ptr());
  const MhaLayout ql = mha_packed_part(s.NH, s.T, s.D);
  const MhaLayout ol = mha_bthd(s.NH, s.T, s.D);
  // the fp32 atomic accumulator only where the launcher cannot prove one key
  // tile per head
  const bool writes_dq = dr_mha_bwd_writes_dq((int)s.T, (int)s.D) != 0;
  at::Tensor dq32;
  if (!writes_dq)
    dq32 = at::zeros({s.B, s.T, s.NH, s.D}, qkv.options().dtype(at::kFloat));
  launch_check(
      dr_mha_bwd(base, base + part, base + 2 * part, o.data_ptr(),
                 dout.data_ptr(), lse.data_ptr<float>(),
                 writes_dq ? (void*)dbase : dq32.data_ptr(), dbase + part,
                 dbase + 2 * part, s.B, (int)s.NH, (int)s.T, (int)s.D,
                 (float)scale, is_bf16(qkv), ql.s, ol.s, writes_dq ? ql.s : ol.s,
                 cur_stream()),
      "dr_mha_bwd");
  if (!writes_dq) dqkv.select(2, 0).copy_(dq32);
  return dqkv;
}

// ----------------------------------------------------------------- sanity
// Normalized model output (N, T, M, 3) + measured utilization (N, T, M) ->
// {scores (N,T,M) f32, flags (N,T,M) u8, max_score, n_flagged, first_flag,
// n_observed (N,M), bands (N,T,M,3) f32 or empty}; semantics in sanity.hip.
// Every operand is checked here: bad input is an exception, never a launch.
// The VALUES of lengths are not read on the host (the kernel clamps them).
std::vector<at::Tensor> band_scores(at::Tensor out, at::Tensor measured,
                                    at::Tensor y_min, at::Tensor y_scale,
                                    c10::optional<at::Tensor> base,
                                    c10::optional<at::Tensor> conformal,
                                    bool log1p,
                                    c10::optional<at::Tensor> lengths,
                                    double threshold, int64_t min_run,
                                    bool want_bands) {
  const at::cuda::CUDAGuard guard(out.device());
  check_dtype(out, "band_scores out");
  TORCH_CHECK(out.is_cuda() && out.dim() == 4 && out.is_contiguous(),
              "band_scores out must be a contiguous (N, T, M, 3) GPU tensor");
  TORCH_CHECK(out.size(3) == 3, "band_scores is defined on the quantile triple: "
              "out must have Q = 3, got ", out.size(3));
  TORCH_CHECK(min_run >= 1 && min_run < (1LL << 31),
              "band_scores min_run must be >= 1, got ", min_run);
  const int64_t N = out.size(0), T = out.size(1), M = out.size(2);
  TORCH_CHECK(T < (1LL << 31) && M < (1LL << 31) && N * M < (1LL << 31) * 64,
              "band_scores shape too large");
  const int64_t ntm[] = {N, T, M}, m1[] = {M};
  check_operand(measured, "band_scores measured", out, at::kFloat, ntm);
  check_operand(y_min, "band_scores y_min", out, at::kFloat, m1);
  check_operand(y_scale, "band_scores y_scale", out, at::kFloat, m1);
  if (base.has_value())
    check_operand(*base, "band_scores base", out, at::kFloat, ntm);
  if (conformal.has_value())
    check_operand(*conformal, "band_scores conformal", out, at::kFloat, m1);
  if (lengths.has_value())
    TORCH_CHECK(lengths->dim() == 1, "band_scores lengths must be (N,)");
  const int* lens = lengths_ptr(lengths, out, N, "band_scores lengths");
  auto f32 = out.options().dtype(at::kFloat);
  auto i32 = out.options().dtype(at::kInt);
  auto scores = at::empty({N, T, M}, f32);
  auto flags = at::empty({N, T, M}, out.options().dtype(at::kByte));
  auto max_score = at::empty({N, M}, f32);
  auto n_flagged = at::empty({N, M}, i32);
  auto first_flag = at::empty({N, M}, i32);
  auto n_observed = at::empty({N, M}, i32);
  auto bands = want_bands ? at::empty({N, T, M, 3}, f32) : at::empty({0}, f32);
  if (N * M == 0) return {scores, flags, max_score, n_flagged, first_flag,
                          n_observed, bands};
  if (T == 0) {                       // nothing to loop over: empty summaries
    max_score.zero_();
    n_flagged.zero_();
    first_flag.fill_(-1);
    n_observed.zero_();
    return {scores, flags, max_score, n_flagged, first_flag, n_observed, bands};
  }
  launch_check(
      dr_sanity_scores(out.data_ptr(), measured.data_ptr<float>(),
                       base.has_value() ? base->data_ptr<float>() : nullptr,
                       y_min.data_ptr<float>(), y_scale.data_ptr<float>(),
                       conformal.has_value() ? conformal->data_ptr<float>()
                                             : nullptr,
                       lens, N, (int)T, (int)M, log1p ? 1 : 0, (float)threshold,
                       (int)min_run, scores.data_ptr<float>(),
                       flags.data_ptr<uint8_t>(), max_score.data_ptr<float>(),
                       n_flagged.data_ptr<int>(), first_flag.data_ptr<int>(),
                       n_observed.data_ptr<int>(),
                       want_bands ? bands.data_ptr<float>() : nullptr,
                       is_bf16(out), cur_stream()),
      "dr_sanity_scores");
  return {scores, flags, max_score, n_flagged, first_flag, n_observed, bands};
}

}  // namespace

void register_featurize(py::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  register_featurize(m);
  m.def("dropout_add_ln_forward", &dropout_add_ln_forward, py::arg("branch"),
        py::arg("residual"), py::arg("weight"), py::arg("bias"), py::arg("seed"),
        py::arg("p"), py::arg("eps"));
  m.def("dropout_add_ln_backward", &dropout_add_ln_backward, py::arg("d_normed"),
        py::arg("d_r_out"), py::arg("r_out"), py::arg("weight"), py::arg("mean"),
        py::arg("rstd"), py::arg("seed"), py::arg("p"));
  m.def("pinball_forward", &pinball_forward);
  m.def("pinball_backward", &pinball_backward);
  m.def("pinball_masked_forward", &pinball_masked_forward);
  m.def("pinball_masked_backward", &pinball_masked_backward);
  m.def("fused_adam", &fused_adam);
  m.def("fused_adam_capturable", &fused_adam_capturable);
  m.def("gru_seq_forward", &gru_seq_forward, py::arg("xg"), py::arg("w_hh"),
        py::arg("b_hh"), py::arg("h0"), py::arg("gamma"), py::arg("beta"),
        py::arg("reverse"), py::arg("save"), py::arg("fp8") = false,
        py::arg("wh_fwd") = py::none(), py::arg("O") = 0);
  m.def("gru_fwd_fuses_heads", &gru_fwd_fuses_heads, py::arg("B"), py::arg("C"),
        py::arg("save"));
  m.def("gru_seq_decode", &gru_seq_decode, py::arg("xg"), py::arg("w_hh"),
        py::arg("b_hh"), py::arg("h0"), py::arg("gamma"), py::arg("beta"),
        py::arg("wh_fwd"), py::arg("O"), py::arg("reverse"), py::arg("fp8") = false,
        py::arg("lengths") = py::none());
  m.def("gru_seq_backward_kernel", &gru_seq_backward_kernel);
  m.def("gru_seq_backward_heads_kernel", &gru_seq_backward_heads_kernel);
  m.def("gru_bwd_reduce", &gru_bwd_reduce, py::arg("dpre"), py::arg("gamma"),
        py::arg("xg"), py::arg("mode") = "auto");
  m.def("gru_reduce_fused_max_c", &dr_gru_reduce_fused_max_c);
  m.def("mha_forward", &mha_forward, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("scale"), py::arg("kv_lengths") = py::none());
  m.def("mha_backward", &mha_backward);
  m.def("mha_packed_forward", &mha_packed_forward, py::arg("qkv"),
        py::arg("n_heads"), py::arg("scale"));
  m.def("mha_packed_backward", &mha_packed_backward, py::arg("qkv"),
        py::arg("n_heads"), py::arg("o"), py::arg("dout"), py::arg("lse"),
        py::arg("scale"));
  m.def("band_scores", &band_scores, py::arg("out"), py::arg("measured"),
        py::arg("y_min"), py::arg("y_scale"), py::arg("base") = py::none(),
        py::arg("conformal") = py::none(), py::arg("log1p") = false,
        py::arg("lengths") = py::none(), py::arg("threshold") = 0.25,
        py::arg("min_run") = 3, py::arg("want_bands") = false);
}
