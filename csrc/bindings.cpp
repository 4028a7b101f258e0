// torch binding layer for paddle_amd._C (compiled host-side by g++;
// kernels live in kernels/*.hip compiled by hipcc for gfx950).
//
// Replaces the reference's pybind layer for our op set
// (paddle/fluid/pybind/eager_functions.cc + generated python_c) -- here
// the autograd glue lives in Python (torch.autograd.Function); this file
// only validates tensors and launches.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "kernels/api.h"

namespace pa {
void mfma_probe(const void* a, const void* bt, float* c, hipStream_t s);
void mfma_probe32(const void* a, const void* bt, float* c, hipStream_t s);
void mfma_probe_fp8mx(const void* a, const void* bt, float* c, int sa, int sb,
                      hipStream_t s);
}

namespace pa_lt {
std::tuple<torch::Tensor, torch::Tensor> fc1_gelu_fwd(
    const torch::Tensor& x, const torch::Tensor& w, const torch::Tensor& bias);
std::tuple<torch::Tensor, torch::Tensor> fc2_dgrad_dgelu(
    const torch::Tensor& dy, const torch::Tensor& w2, const torch::Tensor& z);
int64_t lt_epilogue_probe(int64_t m, int64_t n, int64_t k, int64_t epi);
}  // namespace pa_lt

namespace {

using torch::Tensor;

hipStream_t cur_stream() {
  return (hipStream_t)c10::hip::getCurrentHIPStream().stream();
}

int dt_of(const Tensor& t) {
  switch (t.scalar_type()) {
    case torch::kBFloat16: return pa::kBF16;
    case torch::kFloat: return pa::kF32;
    // no kernel template reads fp16 (pa::kF16 is reserved): the launchers
    // treat "not bf16" as fp32, so a half tensor must never get this far
    default: TORCH_CHECK(false, "unsupported dtype ", t.scalar_type(),
                         " (native kernels take bfloat16 or float32)");
  }
  return -1;
}

#define CHECK_IN(t) \
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), #t " must be contiguous GPU tensor")

// operand handed to a kernel next to x: contiguous GPU tensor of x's dtype
// (the kernels reinterpret every pointer in the dtype of x)
#define CHECK_LIKE(t, x)                                                      \
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&                             \
              t.scalar_type() == x.scalar_type(),                             \
              #t " must be a contiguous GPU tensor with the dtype of " #x)
// same, and the same number of elements (dy, residual, ...)
#define CHECK_SAME(t, x)                                                      \
  do { CHECK_LIKE(t, x);                                                      \
       TORCH_CHECK(t.numel() == x.numel(), #t " must have the size of " #x);  \
  } while (0)
// per-column parameter (weight / bias): dtype of x, d elements
#define CHECK_VEC(t, x, d)                                                    \
  do { CHECK_LIKE(t, x);                                                      \
       TORCH_CHECK(t.numel() == (d), #t " must have ", (d), " elements");     \
  } while (0)
// saved fp32 row statistics
#define CHECK_STAT(t, n)                                                      \
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&                             \
              t.scalar_type() == torch::kFloat && t.numel() == (n),           \
              #t " must be a contiguous fp32 GPU tensor with ", (n), " elements")

// last-dim contract of the 8-wide row kernels
struct Rows { int64_t n, d; };
static Rows check_rows(const Tensor& x, const char* op) {
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, op, ": empty input");
  TORCH_CHECK(x.size(-1) % 8 == 0, op, ": D must be a multiple of 8");
  return {x.numel() / x.size(-1), x.size(-1)};
}

static const void* opt_ptr(const c10::optional<Tensor>& t) {
  return t.has_value() ? t->const_data_ptr() : nullptr;
}

// ---- norms ----------------------------------------------------------------
std::vector<Tensor> layer_norm_fwd(const Tensor& x, const Tensor& w,
                                   const c10::optional<Tensor>& b, double eps) {
  CHECK_IN(x);
  auto [n, d] = check_rows(x, "layer_norm");
  CHECK_VEC(w, x, d);
  if (b.has_value()) CHECK_VEC((*b), x, d);
  auto y = torch::empty_like(x);
  auto mean = torch::empty({n}, x.options().dtype(torch::kFloat));
  auto rstd = torch::empty({n}, x.options().dtype(torch::kFloat));
  pa::layer_norm_fwd(x.const_data_ptr(), w.const_data_ptr(),
                     opt_ptr(b), y.mutable_data_ptr(), mean.mutable_data_ptr<float>(),
                     rstd.mutable_data_ptr<float>(), n, d, (float)eps, dt_of(x),
                     cur_stream());
  return {y, mean, rstd};
}

// h = x + residual, y = LN(h).  d > kLnFusedMaxD runs the two kernels the
// fused one replaces, on the same contract.
std::vector<Tensor> add_layer_norm_fwd(const Tensor& x, const Tensor& residual,
                                       const Tensor& w,
                                       const c10::optional<Tensor>& b, double eps) {
  CHECK_IN(x);
  auto [n, d] = check_rows(x, "add_layer_norm");
  CHECK_SAME(residual, x);
  TORCH_CHECK(residual.sizes() == x.sizes(), "residual must have the shape of x");
  CHECK_VEC(w, x, d);
  if (b.has_value()) CHECK_VEC((*b), x, d);
  auto h = torch::empty_like(x);
  auto y = torch::empty_like(x);
  auto mean = torch::empty({n}, x.options().dtype(torch::kFloat));
  auto rstd = torch::empty({n}, x.options().dtype(torch::kFloat));
  const void* bp = opt_ptr(b);
  if (pa::ln_fused_ok(d)) {
    pa::add_layer_norm_fwd(x.const_data_ptr(), residual.const_data_ptr(),
                           w.const_data_ptr(), bp, h.mutable_data_ptr(),
                           y.mutable_data_ptr(), mean.mutable_data_ptr<float>(),
                           rstd.mutable_data_ptr<float>(), n, d, (float)eps,
                           dt_of(x), cur_stream());
  } else {
    pa::dropout_add_fwd(x.const_data_ptr(), residual.const_data_ptr(),
                        h.mutable_data_ptr(), nullptr, x.numel(), 0.f, 0, 0,
                        dt_of(x), cur_stream());
    pa::layer_norm_fwd(h.const_data_ptr(), w.const_data_ptr(), bp,
                       y.mutable_data_ptr(), mean.mutable_data_ptr<float>(),
                       rstd.mutable_data_ptr<float>(), n, d, (float)eps, dt_of(x),
                       cur_stream());
  }
  return {h, y, mean, rstd};
}

int64_t ln_bwd_grid_cap() { return pa::kLnBwdGridCap; }
bool ln_fused_ok(int64_t d) { return pa::ln_fused_ok(d); }

// dres (optional): residual-stream gradient added to dx in the kernel.
// fused = false, or d > kLnFusedMaxD: the two-kernel path (dx, then dw/db
// from a second read), with dres added by a tensor add.  grid_cap: row-block
// cap of the one-pass kernel, 0 = the measured default.
std::vector<Tensor> layer_norm_bwd(const Tensor& dy, const Tensor& x,
                                   const Tensor& w, const Tensor& mean,
                                   const Tensor& rstd, bool has_bias,
                                   const c10::optional<Tensor>& dres,
                                   bool fused, int64_t grid_cap) {
  CHECK_IN(x);
  auto [n, d] = check_rows(x, "layer_norm_bwd");
  CHECK_SAME(dy, x); CHECK_VEC(w, x, d);
  CHECK_STAT(mean, n); CHECK_STAT(rstd, n);
  if (dres.has_value()) CHECK_SAME((*dres), x);
  TORCH_CHECK(grid_cap >= 0 && grid_cap <= 65536, "layer_norm_bwd: bad grid_cap");
  // dw/db stay fp32: the caller casts them to the parameter's dtype, which
  // under amp O2 is fp32 next to bf16 activations
  auto f32 = x.options().dtype(torch::kFloat);
  auto dx = torch::empty_like(x);
  auto dw = torch::empty({d}, f32);
  auto db = torch::empty({d}, f32);
  if (fused && pa::ln_fused_ok(d)) {
    int grid = pa::ln_bwd_fused_grid(n, (int)grid_cap);
    auto ws = torch::empty({(int64_t)grid * 2 * d}, f32);
    pa::layer_norm_bwd_fused(dy.const_data_ptr(), x.const_data_ptr(),
                             w.const_data_ptr(), mean.const_data_ptr<float>(),
                             rstd.const_data_ptr<float>(), opt_ptr(dres),
                             dx.mutable_data_ptr(), dw.mutable_data_ptr<float>(),
                             db.mutable_data_ptr<float>(),
                             ws.mutable_data_ptr<float>(), grid, n, d, dt_of(x),
                             cur_stream());
    return {dx, dw, db};
  }
  pa::layer_norm_bwd_dx(dy.const_data_ptr(), x.const_data_ptr(), w.const_data_ptr(),
                        mean.const_data_ptr<float>(), rstd.const_data_ptr<float>(),
                        dx.mutable_data_ptr(), n, d, dt_of(x), cur_stream());
  auto ws = torch::empty({(int64_t)pa::col_chunks(n, d) * 2 * d}, f32);
  pa::layer_norm_bwd_dwdb(dy.const_data_ptr(), x.const_data_ptr(),
                          mean.const_data_ptr<float>(), rstd.const_data_ptr<float>(),
                          dw.mutable_data_ptr<float>(), db.mutable_data_ptr<float>(),
                          ws.mutable_data_ptr<float>(), n, d, dt_of(x), cur_stream());
  if (dres.has_value()) dx.add_(dres->view_as(dx));
  return {dx, dw, db};
}

std::vector<Tensor> rms_norm_fwd(const Tensor& x, const c10::optional<Tensor>& residual,
                                 const Tensor& w, double eps) {
  CHECK_IN(x);
  auto [n, d] = check_rows(x, "rms_norm");
  CHECK_VEC(w, x, d);
  auto y = torch::empty_like(x);
  auto rstd = torch::empty({n}, x.options().dtype(torch::kFloat));
  Tensor res_out;
  const void* resp = nullptr;
  void* res_outp = nullptr;
  if (residual.has_value()) {
    CHECK_SAME((*residual), x);
    res_out = torch::empty_like(x);
    resp = residual->const_data_ptr();
    res_outp = res_out.mutable_data_ptr();
  }
  pa::rms_norm_fwd(x.const_data_ptr(), resp, w.const_data_ptr(),
                   y.mutable_data_ptr(), res_outp, rstd.mutable_data_ptr<float>(),
                   n, d, (float)eps, dt_of(x), cur_stream());
  if (residual.has_value()) return {y, rstd, res_out};
  return {y, rstd};
}

std::vector<Tensor> rms_norm_bwd(const Tensor& dy, const Tensor& x, const Tensor& w,
                                 const Tensor& rstd) {
  CHECK_IN(x);
  auto [n, d] = check_rows(x, "rms_norm_bwd");
  CHECK_SAME(dy, x); CHECK_VEC(w, x, d); CHECK_STAT(rstd, n);
  auto f32 = x.options().dtype(torch::kFloat);
  auto dx = torch::empty_like(x);
  auto dw = torch::empty({d}, f32);
  pa::rms_norm_bwd_dx(dy.const_data_ptr(), x.const_data_ptr(), w.const_data_ptr(),
                      rstd.const_data_ptr<float>(), dx.mutable_data_ptr(), n, d,
                      dt_of(x), cur_stream());
  auto ws = torch::empty({(int64_t)pa::col_chunks(n, d) * d}, f32);
  pa::rms_norm_bwd_dw(dy.const_data_ptr(), x.const_data_ptr(),
                      rstd.const_data_ptr<float>(), dw.mutable_data_ptr<float>(),
                      ws.mutable_data_ptr<float>(), n, d, dt_of(x), cur_stream());
  return {dx, dw};  // fp32, cast by the caller
}

// ---- cross entropy --------------------------------------------------------
std::vector<Tensor> softmax_ce_fwd(const Tensor& logits, const Tensor& labels,
                                   int64_t ignore_index) {
  CHECK_IN(logits); CHECK_IN(labels);
  TORCH_CHECK(logits.dim() >= 1 && logits.numel() > 0, "softmax_ce: empty logits");
  int64_t v = logits.size(-1), n = logits.numel() / v;
  TORCH_CHECK(labels.scalar_type() == torch::kLong && labels.numel() == n,
              "softmax_ce: labels must be int64 with one entry per row");
  auto loss = torch::empty({n}, logits.options().dtype(torch::kFloat));
  auto lse = torch::empty({n}, logits.options().dtype(torch::kFloat));
  pa::softmax_ce_fwd(logits.const_data_ptr(), labels.const_data_ptr<int64_t>(),
                     loss.mutable_data_ptr<float>(), lse.mutable_data_ptr<float>(),
                     n, v, ignore_index, dt_of(logits), cur_stream());
  return {loss, lse};
}

Tensor softmax_ce_bwd(const Tensor& dloss, const Tensor& logits,
                      const Tensor& labels, const Tensor& lse, int64_t ignore_index) {
  CHECK_IN(logits); CHECK_IN(labels);
  TORCH_CHECK(logits.dim() >= 1 && logits.numel() > 0, "softmax_ce_bwd: empty logits");
  int64_t v = logits.size(-1), n = logits.numel() / v;
  TORCH_CHECK(labels.scalar_type() == torch::kLong && labels.numel() == n,
              "softmax_ce_bwd: labels must be int64 with one entry per row");
  CHECK_STAT(dloss, n); CHECK_STAT(lse, n);
  auto dlogits = torch::empty_like(logits);
  pa::softmax_ce_bwd(dloss.const_data_ptr<float>(), logits.const_data_ptr(),
                     labels.const_data_ptr<int64_t>(), lse.const_data_ptr<float>(),
                     dlogits.mutable_data_ptr(), n, v, ignore_index, dt_of(logits),
                     cur_stream());
  return dlogits;
}

// ---- elementwise ----------------------------------------------------------
Tensor bias_gelu_fwd(const Tensor& x, const c10::optional<Tensor>& bias) {
  CHECK_IN(x);
  auto [n, d] = check_rows(x, "bias_gelu");
  if (bias.has_value()) CHECK_VEC((*bias), x, d);
  auto y = torch::empty_like(x);
  pa::bias_gelu_fwd(x.const_data_ptr(), opt_ptr(bias), y.mutable_data_ptr(), n, d,
                    dt_of(x), cur_stream());
  return y;
}

Tensor bias_gelu_bwd(const Tensor& dy, const Tensor& x, const c10::optional<Tensor>& bias) {
  CHECK_IN(x);
  auto [n, d] = check_rows(x, "bias_gelu_bwd");
  CHECK_SAME(dy, x);
  if (bias.has_value()) CHECK_VEC((*bias), x, d);
  auto dx = torch::empty_like(x);
  pa::bias_gelu_bwd(dy.const_data_ptr(), x.const_data_ptr(), opt_ptr(bias),
                    dx.mutable_data_ptr(), n, d, dt_of(x), cur_stream());
  return dx;
}

Tensor colsum(const Tensor& x) {
  CHECK_IN(x);
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, "colsum: empty input");
  int64_t d = x.size(-1), n = x.numel() / d;
  auto out = torch::zeros({d}, x.options().dtype(torch::kFloat));
  pa::colsum(x.const_data_ptr(), out.mutable_data_ptr<float>(), n, d, dt_of(x),
             cur_stream());
  return out;
}

// {dx, db}: db fp32 [d] = column sum of dx as stored.  One kernel plus a
// partials reduce when a grid keeps each thread on its columns (fused =
// true and bias_gelu_bwd_db_grid > 0), else bias_gelu_bwd then colsum.
std::vector<Tensor> bias_gelu_bwd_db(const Tensor& dy, const Tensor& x,
                                     const c10::optional<Tensor>& bias, bool fused) {
  CHECK_IN(x);
  auto [n, d] = check_rows(x, "bias_gelu_bwd_db");
  CHECK_SAME(dy, x);
  if (bias.has_value()) CHECK_VEC((*bias), x, d);
  const void* bp = opt_ptr(bias);
  auto dx = torch::empty_like(x);
  int grid = fused ? pa::bias_gelu_bwd_db_grid(n, d) : 0;
  if (grid > 0) {
    const int64_t w = d % 16 == 0 ? 16 : 8;
    auto db = torch::empty({d}, x.options().dtype(torch::kFloat));
    auto ws = torch::empty({(int64_t)grid * 256 * w}, x.options().dtype(torch::kFloat));
    pa::bias_gelu_bwd_db(dy.const_data_ptr(), x.const_data_ptr(), bp,
                         dx.mutable_data_ptr(), db.mutable_data_ptr<float>(),
                         ws.mutable_data_ptr<float>(), grid, n, d, dt_of(x),
                         cur_stream());
    return {dx, db};
  }
  pa::bias_gelu_bwd(dy.const_data_ptr(), x.const_data_ptr(), bp,
                    dx.mutable_data_ptr(), n, d, dt_of(x), cur_stream());
  return {dx, colsum(dx)};
}

bool bias_gelu_bwd_db_fused(int64_t n, int64_t d) {
  return pa::bias_gelu_bwd_db_grid(n, d) > 0;
}

Tensor swiglu_fwd(const Tensor& x) {
  CHECK_IN(x);
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, "swiglu: empty input");
  int64_t d2 = x.size(-1), n = x.numel() / d2, d = d2 / 2;
  TORCH_CHECK(d2 % 16 == 0, "swiglu: last dim must be a multiple of 16");
  auto sizes = x.sizes().vec();
  sizes.back() = d;
  auto y = torch::empty(sizes, x.options());
  pa::swiglu_fwd(x.const_data_ptr(), y.mutable_data_ptr(), n, d, dt_of(x), cur_stream());
  return y;
}

Tensor swiglu_bwd(const Tensor& dy, const Tensor& x) {
  CHECK_IN(x);
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, "swiglu_bwd: empty input");
  int64_t d2 = x.size(-1), n = x.numel() / d2, d = d2 / 2;
  TORCH_CHECK(d2 % 16 == 0, "swiglu_bwd: last dim must be a multiple of 16");
  CHECK_LIKE(dy, x);
  TORCH_CHECK(dy.numel() == n * d, "swiglu_bwd: dy must have half the size of x");
  auto dx = torch::empty_like(x);
  pa::swiglu_bwd(dy.const_data_ptr(), x.const_data_ptr(), dx.mutable_data_ptr(),
                 n, d, dt_of(x), cur_stream());
  return dx;
}

Tensor rope_fwd(const Tensor& x, const Tensor& cos_t, const Tensor& sin_t,
                int64_t pos_offset, bool conj) {
  CHECK_IN(x); CHECK_IN(cos_t); CHECK_IN(sin_t);
  TORCH_CHECK(x.dim() == 4, "rope expects [B,S,H,D]");
  int64_t b = x.size(0), sl = x.size(1), h = x.size(2), dh = x.size(3);
  TORCH_CHECK(dh % 2 == 0 && (dh / 2) % 4 == 0 && x.numel() > 0,
              "rope: head_dim/2 must be multiple of 4");
  TORCH_CHECK(pos_offset >= 0, "rope: pos_offset must be >= 0");
  TORCH_CHECK(cos_t.scalar_type() == torch::kFloat &&
              sin_t.scalar_type() == torch::kFloat &&
              cos_t.dim() == 2 && sin_t.dim() == 2 &&
              cos_t.size(1) == dh / 2 && sin_t.size(1) == dh / 2 &&
              cos_t.size(0) >= sl + pos_offset && sin_t.size(0) >= sl + pos_offset,
              "rope: cos/sin must be fp32 [>= seq_len + pos_offset, head_dim/2]");
  auto y = torch::empty_like(x);
  pa::rope_fwd(x.const_data_ptr(), cos_t.const_data_ptr<float>(),
               sin_t.const_data_ptr<float>(), y.mutable_data_ptr(), b, sl, h, dh,
               pos_offset, conj, dt_of(x), cur_stream());
  return y;
}

// ---- adamw ----------------------------------------------------------------
void adamw(Tensor& master, c10::optional<Tensor> param_out, const Tensor& grad,
           Tensor& m, Tensor& v, double lr, double beta1, double beta2,
           double eps, double wd, double beta1_pow, double beta2_pow,
           double grad_scale) {
  CHECK_IN(master); CHECK_IN(grad); CHECK_IN(m); CHECK_IN(v);
  int64_t numel = master.numel();
  TORCH_CHECK(master.scalar_type() == torch::kFloat &&
              m.scalar_type() == torch::kFloat && v.scalar_type() == torch::kFloat,
              "adamw: master, m and v must be fp32");
  TORCH_CHECK(grad.numel() == numel && m.numel() == numel && v.numel() == numel,
              "adamw: grad, m and v must have the size of master");
  bool bf16out = false;
  void* pout = nullptr;
  if (param_out.has_value()) {
    TORCH_CHECK(param_out->is_cuda() && param_out->is_contiguous() &&
                param_out->numel() == numel &&
                (param_out->scalar_type() == torch::kBFloat16 ||
                 param_out->scalar_type() == torch::kFloat),
                "adamw: param_out must be a contiguous bf16 or fp32 GPU tensor "
                "with the size of master");
    bf16out = param_out->scalar_type() == torch::kBFloat16;
    pout = param_out->mutable_data_ptr();
  }
  pa::adamw(master.mutable_data_ptr<float>(), pout, grad.const_data_ptr(),
            m.mutable_data_ptr<float>(), v.mutable_data_ptr<float>(), numel,
            (float)lr, (float)beta1, (float)beta2, (float)eps, (float)wd,
            (float)beta1_pow, (float)beta2_pow, (float)grad_scale,
            dt_of(grad), bf16out, cur_stream());
}

Tensor l2norm_sq(const Tensor& x) {
  CHECK_IN(x);
  auto out = torch::zeros({1}, x.options().dtype(torch::kFloat));
  pa::l2norm_sq(x.const_data_ptr(), out.mutable_data_ptr<float>(), x.numel(),
                dt_of(x), cur_stream());
  return out;
}

// ---- flash attention ------------------------------------------------------
// Dense tensors are logical [B, H, S, D] but may be strided VIEWS (e.g. of a
// packed [B, S, 3, H, D] qkv) as long as D is contiguous and rows are
// 16B-aligned.  Every check runs before anything is launched.
static pa::FaStride fa_view(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 && t.dim() == 4,
              "flash_attn: ", name, " must be a bf16 GPU tensor [B, H, S, D]");
  TORCH_CHECK(t.stride(3) == 1, "flash_attn: ", name, ": head_dim must be contiguous");
  TORCH_CHECK(t.stride(2) % 8 == 0,
              "flash_attn: ", name, ": seq stride must keep 16B alignment");
  return {t.stride(0), t.stride(1), t.stride(2)};
}

static bool fa_same(const pa::FaStride& x, const pa::FaStride& y) {
  return x.b == y.b && x.h == y.h && x.s == y.s;
}

// GQA backward: G = gqa_heads_per_block q heads per dK/dV block (0 = the whole
// group of h / hkv).  Below the group size the blocks write fp32 partials,
// which this allocates; the returned tensor must outlive the launch.
static Tensor fa_gqa_setup(pa::FaArgs& a, int64_t gqa_heads_per_block, const Tensor& like) {
  const int64_t rep = a.h / a.hkv;
  TORCH_CHECK(gqa_heads_per_block >= 0 &&
              (gqa_heads_per_block == 0 || rep % gqa_heads_per_block == 0),
              "flash_attn_bwd: gqa_heads_per_block must be 0 or divide H / HKV (", rep, ")");
  TORCH_CHECK(a.hkv == a.h || a.mask == nullptr,
              "flash_attn_bwd: hkv != h with a mask has no kernel (expand KV upstream)");
  a.gqa_heads = (int)gqa_heads_per_block;
  Tensor ws;
  if (a.gqa_heads != 0 && a.gqa_heads != rep) {
    ws = torch::empty({2, (int64_t)a.b * (a.h / a.gqa_heads), a.skv, a.dh},
                      like.options().dtype(torch::kFloat));
    a.gqa_ws = ws.mutable_data_ptr<float>();
  }
  return ws;
}

static pa::FaStride fa_mask_strides(const Tensor& m, int64_t b, int64_t h,
                                    int64_t sq, int64_t skv) {
  TORCH_CHECK(m.dim() == 4 && m.size(3) == skv && m.size(2) == sq &&
              (m.size(1) == 1 || m.size(1) == h) &&
              (m.size(0) == 1 || m.size(0) == b),
              "flash_attn mask must be [B|1, H|1, Sq, Skv]");
  TORCH_CHECK(m.is_cuda() && m.stride(3) == 1 && m.scalar_type() == torch::kBFloat16,
              "flash_attn mask: bf16 on the GPU with contiguous last dim");
  return {m.size(0) == 1 ? 0 : m.stride(0), m.size(1) == 1 ? 0 : m.stride(1),
          m.stride(2)};
}

// what forward and backward share: q / k / v, the mask and the scalars
static pa::FaArgs fa_dense_args(const Tensor& q, const Tensor& k, const Tensor& v,
                                double scale, bool causal,
                                const c10::optional<Tensor>& mask, double pdrop,
                                int64_t seed, int64_t offset) {
  pa::FaArgs a{};
  a.q_s = fa_view(q, "q");
  a.k_s = fa_view(k, "k");
  TORCH_CHECK(fa_same(a.k_s, fa_view(v, "v")), "flash_attn: k/v must share strides");
  a.b = (int)q.size(0); a.h = (int)q.size(1); a.sq = (int)q.size(2); a.dh = (int)q.size(3);
  a.hkv = (int)k.size(1); a.skv = (int)k.size(2);
  TORCH_CHECK(a.dh == 128 || a.dh == 64, "flash_attn: head_dim must be 64/128");
  TORCH_CHECK(k.size(0) == a.b && k.size(3) == a.dh && v.sizes() == k.sizes(),
              "flash_attn: k and v must be [B, HKV, Skv, D] with q's B and D");
  TORCH_CHECK(a.hkv > 0 && a.h % a.hkv == 0, "flash_attn: H must be a multiple of HKV");
  if (mask.has_value()) {
    a.m_s = fa_mask_strides(*mask, a.b, a.h, a.sq, a.skv);
    a.mask = mask->const_data_ptr();
  }
  a.q = q.const_data_ptr(); a.k = k.const_data_ptr(); a.v = v.const_data_ptr();
  a.scale = (float)scale; a.causal = causal;
  a.pdrop = (float)pdrop; a.seed = (uint64_t)seed; a.offset = (uint64_t)offset;
  return a;
}

std::vector<Tensor> flash_attn_fwd(const Tensor& q, const Tensor& k, const Tensor& v,
                                   c10::optional<Tensor> o_out,
                                   double scale, bool causal,
                                   c10::optional<Tensor> mask,
                                   double pdrop, int64_t seed, int64_t offset) {
  pa::FaArgs a = fa_dense_args(q, k, v, scale, causal, mask, pdrop, seed, offset);
  auto o = o_out.has_value() ? *o_out : torch::empty({a.b, a.h, a.sq, a.dh}, q.options());
  a.o_s = fa_view(o, "o");
  TORCH_CHECK(o.sizes() == q.sizes(), "flash_attn: o must have q's shape");
  auto lse = torch::empty({a.b, a.h, a.sq}, q.options().dtype(torch::kFloat));
  a.o = o.mutable_data_ptr();
  a.lse = lse.mutable_data_ptr<float>();
  pa::flash_attn_fwd(a, cur_stream());
  return {o, lse};
}

std::vector<Tensor> flash_attn_bwd(const Tensor& dout, const Tensor& q, const Tensor& k,
                                   const Tensor& v, const Tensor& o, const Tensor& lse,
                                   c10::optional<Tensor> dq_out,
                                   c10::optional<Tensor> dk_out,
                                   c10::optional<Tensor> dv_out,
                                   double scale, bool causal,
                                   c10::optional<Tensor> mask,
                                   double pdrop, int64_t seed, int64_t offset,
                                   int64_t gqa_heads_per_block) {
  pa::FaArgs a = fa_dense_args(q, k, v, scale, causal, mask, pdrop, seed, offset);
  auto dq = dq_out.has_value() ? *dq_out : torch::empty({a.b, a.h, a.sq, a.dh}, q.options());
  auto dk = dk_out.has_value() ? *dk_out : torch::empty({a.b, a.hkv, a.skv, a.dh}, k.options());
  auto dv = dv_out.has_value() ? *dv_out : torch::empty({a.b, a.hkv, a.skv, a.dh}, v.options());
  a.do_s = fa_view(dout, "dout");
  a.o_s = fa_view(o, "o");
  a.dq_s = fa_view(dq, "dq");
  a.dk_s = fa_view(dk, "dk");
  TORCH_CHECK(fa_same(a.dk_s, fa_view(dv, "dv")), "flash_attn_bwd: dk/dv must share strides");
  TORCH_CHECK(dout.sizes() == q.sizes() && o.sizes() == q.sizes() && dq.sizes() == q.sizes(),
              "flash_attn_bwd: dout, o and dq must have q's shape");
  TORCH_CHECK(dk.sizes() == k.sizes() && dv.sizes() == k.sizes(),
              "flash_attn_bwd: dk and dv must have k's shape");
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == torch::kFloat && lse.is_contiguous() &&
              lse.sizes() == at::IntArrayRef({a.b, a.h, a.sq}),
              "flash_attn_bwd: lse must be fp32 contiguous [B, H, Sq] on the GPU");
  auto delta = torch::empty_like(lse);
  a.dout = dout.const_data_ptr();
  a.o = const_cast<void*>(o.const_data_ptr());
  a.lse = const_cast<float*>(lse.const_data_ptr<float>());
  a.delta = delta.mutable_data_ptr<float>();
  a.dq = dq.mutable_data_ptr(); a.dk = dk.mutable_data_ptr(); a.dv = dv.mutable_data_ptr();
  Tensor ws = fa_gqa_setup(a, gqa_heads_per_block, q);
  pa::flash_attn_bwd(a, cur_stream());
  return {dq, dk, dv};
}

// delta[b, h, sq] = rowsum(dout * o): the first kernel of flash_attn_bwd on
// its own.  dout / o: bf16 [b, h, sq, d] views with head_dim contiguous.
Tensor flash_attn_bwd_delta(const Tensor& dout, const Tensor& o) {
  TORCH_CHECK(dout.is_cuda() && o.is_cuda() &&
              dout.scalar_type() == torch::kBFloat16 &&
              o.scalar_type() == torch::kBFloat16 && dout.dim() == 4 &&
              dout.sizes() == o.sizes() && dout.numel() > 0,
              "flash_attn_bwd_delta: dout / o must be bf16 [b, h, sq, d] GPU tensors of one shape");
  int64_t b = o.size(0), h = o.size(1), sq = o.size(2), d = o.size(3);
  TORCH_CHECK(d == 128 || d == 64, "flash_attn_bwd_delta: head_dim must be 64 or 128");
  const pa::FaStride dos = fa_view(dout, "dout"), os = fa_view(o, "o");
  for (long long st : {dos.b, dos.h, dos.s, os.b, os.h, os.s})
    TORCH_CHECK(st % 8 == 0 && st >= 0,
                "flash_attn_bwd_delta: strides must keep rows 16-byte aligned");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(dout.const_data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(o.const_data_ptr()) % 16 == 0,
              "flash_attn_bwd_delta: 16-byte aligned data required");
  auto delta = torch::empty({b, h, sq}, o.options().dtype(torch::kFloat));
  pa::flash_attn_bwd_delta(dout.const_data_ptr(), o.const_data_ptr(),
                           delta.mutable_data_ptr<float>(), b, h, sq, d, dos, os,
                           cur_stream());
  return delta;
}

// host-side block map for the varlen kernels: (seq, offset) per block
static std::pair<Tensor, int64_t> make_bmap(const Tensor& cu_cpu, int64_t blk) {
  auto acc = cu_cpu.accessor<int, 1>();
  std::vector<int> map;
  for (int64_t i = 0; i + 1 < cu_cpu.size(0); ++i) {
    int len = acc[i + 1] - acc[i];
    for (int off = 0; off < len; off += (int)blk) {
      map.push_back((int)i);
      map.push_back(off);
    }
  }
  auto t = torch::from_blob(map.data(), {(int64_t)map.size()},
                            torch::dtype(torch::kInt32)).clone().cuda();
  return {t, (int64_t)map.size() / 2};
}

// Varlen: q / k / v packed [total, H, D] contiguous, cu_q / cu_k int32
// [nseq + 1] prefix sums.  Fills the shared part of FaArgs; `keep` holds the
// device tensors the launch reads.
static pa::FaArgs fa_varlen_args(const Tensor& q, const Tensor& k, const Tensor& v,
                                 const Tensor& cu_q, const Tensor& cu_k, double scale,
                                 bool causal, double pdrop, int64_t seed, int64_t offset,
                                 bool bwd, std::vector<Tensor>& keep) {
  for (const Tensor* t : {&q, &k, &v})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kBFloat16 && t->dim() == 3 &&
                t->is_contiguous(),
                "flash_attn_varlen: q, k, v must be contiguous bf16 GPU tensors [total, H, D]");
  pa::FaArgs a{};
  a.b = 1; a.h = (int)q.size(1); a.hkv = (int)k.size(1); a.dh = (int)q.size(2);
  a.sq = (int)q.size(0); a.skv = (int)k.size(0);
  TORCH_CHECK(a.dh == 128 || a.dh == 64, "flash_attn_varlen: head_dim must be 64/128");
  TORCH_CHECK(k.size(2) == a.dh && v.sizes() == k.sizes(),
              "flash_attn_varlen: k and v must be [total_k, HKV, D] with q's D");
  TORCH_CHECK(a.hkv > 0 && a.h % a.hkv == 0,
              "flash_attn_varlen: H must be a multiple of HKV");
  TORCH_CHECK(cu_q.scalar_type() == torch::kInt32 && cu_k.scalar_type() == torch::kInt32 &&
              cu_q.dim() == 1 && cu_k.dim() == 1 && cu_q.size(0) == cu_k.size(0) &&
              cu_q.size(0) >= 2,
              "flash_attn_varlen: cu_seqlens must be int32 [nseq + 1] of one length");
  auto cu_q_cpu = cu_q.cpu().contiguous();
  auto cu_k_cpu = cu_k.cpu().contiguous();
  const int64_t n = cu_q.size(0);
  TORCH_CHECK(cu_q_cpu.const_data_ptr<int>()[n - 1] == a.sq &&
              cu_k_cpu.const_data_ptr<int>()[n - 1] == a.skv,
              "flash_attn_varlen: the last cu_seqlens entries must be the packed totals");
  keep.push_back(cu_q.is_cuda() ? cu_q.contiguous() : cu_q_cpu.cuda());
  keep.push_back(cu_k.is_cuda() ? cu_k.contiguous() : cu_k_cpu.cuda());
  a.cu_q = keep[0].const_data_ptr<int>();
  a.cu_k = keep[1].const_data_ptr<int>();
  auto [qb, nqb] = make_bmap(cu_q_cpu, 128);
  keep.push_back(qb);
  a.q_bmap = qb.const_data_ptr<int>(); a.n_qblocks = (int)nqb;
  if (bwd) {
    auto [kb, nkb] = make_bmap(cu_k_cpu, 128);
    keep.push_back(kb);
    a.kv_bmap = kb.const_data_ptr<int>(); a.n_kvblocks = (int)nkb;
  }
  const pa::FaStride qs{0, a.dh, (long long)a.h * a.dh}, ks{0, a.dh, (long long)a.hkv * a.dh};
  a.q_s = a.o_s = a.do_s = a.dq_s = qs;
  a.k_s = a.dk_s = ks;
  a.q = q.const_data_ptr(); a.k = k.const_data_ptr(); a.v = v.const_data_ptr();
  a.scale = (float)scale; a.causal = causal;
  a.pdrop = (float)pdrop; a.seed = (uint64_t)seed; a.offset = (uint64_t)offset;
  return a;
}

std::vector<Tensor> flash_attn_varlen_fwd(const Tensor& q, const Tensor& k,
                                          const Tensor& v, const Tensor& cu_q,
                                          const Tensor& cu_k, double scale,
                                          bool causal, double pdrop,
                                          int64_t seed, int64_t offset) {
  std::vector<Tensor> keep;
  pa::FaArgs a = fa_varlen_args(q, k, v, cu_q, cu_k, scale, causal, pdrop, seed, offset,
                                false, keep);
  auto o = torch::empty_like(q);
  auto lse = torch::empty({a.h, a.sq}, q.options().dtype(torch::kFloat));
  a.o = o.mutable_data_ptr();
  a.lse = lse.mutable_data_ptr<float>();
  pa::flash_attn_fwd(a, cur_stream());
  return {o, lse};
}

std::vector<Tensor> flash_attn_varlen_bwd(const Tensor& dout, const Tensor& q,
                                          const Tensor& k, const Tensor& v,
                                          const Tensor& o, const Tensor& lse,
                                          const Tensor& cu_q, const Tensor& cu_k,
                                          double scale, bool causal,
                                          double pdrop, int64_t seed,
                                          int64_t offset,
                                          int64_t gqa_heads_per_block) {
  std::vector<Tensor> keep;
  pa::FaArgs a = fa_varlen_args(q, k, v, cu_q, cu_k, scale, causal, pdrop, seed, offset,
                                true, keep);
  auto doc = dout.contiguous();
  for (const Tensor* t : std::initializer_list<const Tensor*>{&doc, &o})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kBFloat16 && t->is_contiguous() &&
                t->sizes() == q.sizes(),
                "flash_attn_varlen_bwd: dout and o must be bf16 GPU tensors of q's shape, o contiguous");
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == torch::kFloat && lse.is_contiguous() &&
              lse.sizes() == at::IntArrayRef({a.h, a.sq}),
              "flash_attn_varlen_bwd: lse must be fp32 contiguous [H, total_q] on the GPU");
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  auto delta = torch::empty_like(lse);
  a.dout = doc.const_data_ptr();
  a.o = const_cast<void*>(o.const_data_ptr());
  a.lse = const_cast<float*>(lse.const_data_ptr<float>());
  a.delta = delta.mutable_data_ptr<float>();
  a.dq = dq.mutable_data_ptr(); a.dk = dk.mutable_data_ptr(); a.dv = dv.mutable_data_ptr();
  Tensor ws = fa_gqa_setup(a, gqa_heads_per_block, q);
  pa::flash_attn_bwd(a, cur_stream());
  return {dq, dk, dv};
}

Tensor fa_dropout_mask(int64_t b, int64_t h, int64_t sq, int64_t skv,
                       double p, int64_t seed, int64_t offset) {
  auto out = torch::empty({b, h, sq, skv},
                          torch::dtype(torch::kUInt8).device(torch::kCUDA));
  pa::fa_dropout_mask(out.mutable_data_ptr(), out.numel(), (float)p,
                      (uint64_t)seed, (uint64_t)offset, cur_stream());
  return out;
}

// ---- dropout_add ----------------------------------------------------------
std::vector<Tensor> dropout_add_fwd(const Tensor& x, const c10::optional<Tensor>& residual,
                                    double p, int64_t seed, int64_t offset) {
  CHECK_IN(x);
  TORCH_CHECK(x.numel() > 0 && x.numel() % 8 == 0,
              "dropout_add: numel must be a multiple of 8");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_add: p must be in [0, 1)");
  if (residual.has_value()) CHECK_SAME((*residual), x);
  auto y = torch::empty_like(x);
  Tensor mask;
  uint8_t* maskp = nullptr;
  if (p > 0) {
    mask = torch::empty(x.sizes(), x.options().dtype(torch::kUInt8));
    maskp = mask.mutable_data_ptr<uint8_t>();
  }
  pa::dropout_add_fwd(x.const_data_ptr(), opt_ptr(residual),
                      y.mutable_data_ptr(), maskp, x.numel(), (float)p,
                      (uint64_t)seed, (uint64_t)offset, dt_of(x), cur_stream());
  if (p > 0) return {y, mask};
  return {y};
}

Tensor dropout_add_bwd(const Tensor& dy, const Tensor& mask, double p) {
  CHECK_IN(dy); CHECK_IN(mask);
  TORCH_CHECK(dy.numel() > 0 && dy.numel() % 8 == 0,
              "dropout_add_bwd: numel must be a multiple of 8");
  TORCH_CHECK(mask.scalar_type() == torch::kUInt8 && mask.numel() == dy.numel(),
              "dropout_add_bwd: mask must be uint8 with the size of dy");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_add_bwd: p must be in [0, 1)");
  auto dx = torch::empty_like(dy);
  pa::dropout_add_bwd(dy.const_data_ptr(), mask.const_data_ptr<uint8_t>(),
                      dx.mutable_data_ptr(), dy.numel(), (float)p, dt_of(dy),
                      cur_stream());
  return dx;
}

// ---- embedding ------------------------------------------------------------
Tensor embedding_fwd(const Tensor& table, const Tensor& ids_in, int64_t padding_idx) {
  CHECK_IN(table);
  TORCH_CHECK(ids_in.is_cuda(), "ids must be on GPU");
  TORCH_CHECK(ids_in.scalar_type() == torch::kLong, "embedding: ids must be int64");
  TORCH_CHECK(table.dim() == 2 && table.numel() > 0, "embedding: table must be [vocab, D]");
  auto ids = ids_in.contiguous();
  int64_t vocab = table.size(0), d = table.size(1), n = ids.numel();
  TORCH_CHECK(d % 8 == 0, "embedding: D must be a multiple of 8");
  auto sizes = ids.sizes().vec();
  sizes.push_back(d);
  auto out = torch::empty(sizes, table.options());
  pa::embedding_fwd(table.const_data_ptr(), ids.const_data_ptr<int64_t>(),
                    out.mutable_data_ptr(), n, d, vocab, padding_idx,
                    dt_of(table), cur_stream());
  return out;
}

Tensor embedding_bwd(const Tensor& dout, const Tensor& ids_in, int64_t vocab,
                     int64_t padding_idx) {
  CHECK_IN(dout);
  TORCH_CHECK(ids_in.is_cuda(), "ids must be on GPU");
  TORCH_CHECK(ids_in.scalar_type() == torch::kLong, "embedding_bwd: ids must be int64");
  auto ids = ids_in.contiguous();
  TORCH_CHECK(dout.dim() >= 1 && dout.numel() > 0 && vocab > 0, "embedding_bwd: empty input");
  int64_t d = dout.size(-1), n = ids.numel();
  TORCH_CHECK(d % 8 == 0, "embedding_bwd: D must be a multiple of 8");
  TORCH_CHECK(dout.numel() == n * d, "embedding_bwd: dout must be [ids..., D]");
  auto dtable = torch::zeros({vocab, d}, dout.options().dtype(torch::kFloat));
  pa::embedding_bwd(dout.const_data_ptr(), ids.const_data_ptr<int64_t>(),
                    dtable.mutable_data_ptr<float>(), n, d, vocab, padding_idx,
                    dt_of(dout), cur_stream());
  return dtable;
}

// ---- int8 paged KV cache ---------------------------------------------------
// Contract shared by kv_quant_append and decode_attention_int8 (docs/
// KERNELS.md): int8 contiguous [nblocks, bs, HKV, D] code pools of equal
// shape, D in {64, 128}; fp32 contiguous scales, both [nblocks, bs, HKV]
// (per token) or both [HKV] (per head).  Returns true for per-token scales.
static bool check_kv_int8_pools(const Tensor& kcache, const Tensor& vcache,
                                const Tensor& kscale, const Tensor& vscale,
                                const at::Device& dev, const char* op) {
  for (const Tensor* t : {&kcache, &vcache, &kscale, &vscale})
    TORCH_CHECK(t->is_cuda() && t->device() == dev, op,
                ": all tensors must be on one GPU");
  TORCH_CHECK(kcache.scalar_type() == torch::kChar &&
              vcache.scalar_type() == torch::kChar, op, ": caches must be int8");
  TORCH_CHECK(kcache.dim() == 4 && kcache.is_contiguous() &&
              vcache.is_contiguous() && kcache.sizes() == vcache.sizes(), op,
              ": caches must be contiguous [nblocks, block_size, HKV, D] of "
              "equal shape");
  const int64_t d = kcache.size(3);
  TORCH_CHECK(d == 64 || d == 128, op, ": D must be 64 or 128, got ", d);
  TORCH_CHECK(kcache.numel() > 0, op, ": empty cache");
  TORCH_CHECK(kscale.scalar_type() == torch::kFloat &&
              vscale.scalar_type() == torch::kFloat &&
              kscale.is_contiguous() && vscale.is_contiguous(), op,
              ": scales must be contiguous float32");
  TORCH_CHECK(kscale.sizes() == vscale.sizes(), op,
              ": k_scale and v_scale must be of the same kind");
  const bool per_token = kscale.dim() == 3;
  if (per_token) {
    TORCH_CHECK(kscale.size(0) == kcache.size(0) &&
                kscale.size(1) == kcache.size(1) &&
                kscale.size(2) == kcache.size(2), op,
                ": per-token scales must be [nblocks, block_size, HKV]");
  } else {
    TORCH_CHECK(kscale.dim() == 1 && kscale.size(0) == kcache.size(2), op,
                ": scales must be [nblocks, block_size, HKV] or [HKV]");
  }
  return per_token;
}

void kv_quant_append(const Tensor& k, const Tensor& v, const Tensor& kcache,
                     const Tensor& vcache, const Tensor& kscale,
                     const Tensor& vscale,
                     const Tensor& blk, const Tensor& off,
                     const c10::optional<Tensor>& k_qscale,
                     const c10::optional<Tensor>& v_qscale) {
  const char* op = "kv_quant_append";
  TORCH_CHECK(k.is_cuda(), op, ": k must be a GPU tensor");
  const bool per_token =
      check_kv_int8_pools(kcache, vcache, kscale, vscale, k.device(), op);
  const int64_t bs = kcache.size(1), hkv = kcache.size(2), d = kcache.size(3);
  for (const Tensor* t : {&k, &v}) {
    TORCH_CHECK(t->is_cuda() && t->device() == k.device(), op,
                ": all tensors must be on one GPU");
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16 && t->dim() == 3, op,
                ": k/v must be bfloat16 [T, HKV, D]");
    TORCH_CHECK(t->size(0) == k.size(0) && t->size(1) == hkv && t->size(2) == d,
                op, ": k/v must be [T, HKV, D] matching the cache");
    TORCH_CHECK(t->stride(2) == 1 && t->stride(0) % 8 == 0 &&
                t->stride(1) % 8 == 0 && t->stride(0) >= 0 && t->stride(1) >= 0,
                op, ": k/v need contiguous D and token/head strides % 8 == 0");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->const_data_ptr()) % 16 == 0, op,
                ": k/v must start 16-byte aligned");
  }
  const int64_t t = k.size(0);
  for (const Tensor* i : {&blk, &off})
    TORCH_CHECK(i->is_cuda() && i->device() == k.device() &&
                i->scalar_type() == torch::kLong && i->dim() == 1 &&
                i->size(0) == t && i->is_contiguous(), op,
                ": blk/off must be contiguous int64 [T] on k's device");
  TORCH_CHECK(k_qscale.has_value() == v_qscale.has_value(), op,
              ": give both quant scales or neither");
  const float *kq = nullptr, *vq = nullptr;
  if (k_qscale.has_value()) {
    TORCH_CHECK(!per_token, op,
                ": fixed quant scales go with per-head [HKV] dequant scales");
    for (const Tensor* q : {&*k_qscale, &*v_qscale})
      TORCH_CHECK(q->is_cuda() && q->device() == k.device() &&
                  q->scalar_type() == torch::kFloat && q->dim() == 1 &&
                  q->size(0) == hkv && q->is_contiguous(), op,
                  ": quant scales must be contiguous float32 [HKV]");
    kq = k_qscale->const_data_ptr<float>();
    vq = v_qscale->const_data_ptr<float>();
  } else {
    TORCH_CHECK(per_token, op,
                ": per-head [HKV] scales need k_qscale/v_qscale");
  }
  pa::kv_quant_append(k.const_data_ptr(), v.const_data_ptr(),
                      kcache.mutable_data_ptr(), vcache.mutable_data_ptr(),
                      kscale.mutable_data_ptr<float>(),
                      vscale.mutable_data_ptr<float>(),
                      blk.const_data_ptr<int64_t>(),
                      off.const_data_ptr<int64_t>(), kq, vq, t, hkv, d, bs,
                      kcache.size(0), k.stride(0), k.stride(1), v.stride(0),
                      v.stride(1), cur_stream());
}

// ---- paged decode attention ------------------------------------------------
// The one contract of decode_attention, decode_attention_int8 and
// decode_attention_split (docs/KERNELS.md "paged decode attention"); returns
// the launch arguments, to which the caller adds scale, output and
// workspaces.  Every check precedes any launch.  `dense` is null for the
// paged layout [nblocks, bs, HKV, D]; else {blk, pos, head, bs}: the caller's
// element strides and block size over bf16 caches [nblocks, HKV, ., D].
// `batch` is null where q is [B, H, D]; paged_prefill_attention passes its B
// for q [T, H, D].
static pa::DecodeAttnArgs check_paged_decode(
    const char* op, const Tensor& q, const Tensor& kcache,
    const Tensor& vcache, const Tensor& block_table, const Tensor& seq_lens,
    const c10::optional<Tensor>& k_scale, const c10::optional<Tensor>& v_scale,
    int64_t nsplit, const int64_t* dense = nullptr,
    const int64_t* batch = nullptr) {
  TORCH_CHECK(q.is_cuda(), op, ": q must be a GPU tensor");
  TORCH_CHECK(k_scale.has_value() == v_scale.has_value(), op,
              ": give both k_scale and v_scale or neither");
  const bool int8 = k_scale.has_value();
  bool per_token = false;
  if (int8) {
    per_token = check_kv_int8_pools(kcache, vcache, *k_scale, *v_scale,
                                    q.device(), op);
  } else {
    for (const Tensor* t : {&kcache, &vcache})
      TORCH_CHECK(t->is_cuda() && t->device() == q.device(), op,
                  ": all tensors must be on one GPU");
    TORCH_CHECK(kcache.scalar_type() == torch::kBFloat16 &&
                vcache.scalar_type() == torch::kBFloat16, op,
                ": caches must be bfloat16 (or int8 with scales)");
    TORCH_CHECK(kcache.dim() == 4 && kcache.is_contiguous() &&
                vcache.is_contiguous() && kcache.sizes() == vcache.sizes(), op,
                ": caches must be contiguous [nblocks, block_size, HKV, D] of "
                "equal shape");
    TORCH_CHECK(kcache.size(3) == 64 || kcache.size(3) == 128, op,
                ": D must be 64 or 128, got ", kcache.size(3));
    TORCH_CHECK(kcache.numel() > 0, op, ": empty cache");
  }
  for (const Tensor* t : {&kcache, &vcache})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->const_data_ptr()) % 16 == 0, op,
                ": caches must start 16-byte aligned");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 && q.dim() == 3 &&
              q.is_contiguous(), op, ": q must be contiguous bfloat16 [B, H, D]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.const_data_ptr()) % 16 == 0, op,
              ": q must start 16-byte aligned");
  // prefill: q is [T, H, D] and the batch is the table's
  const int64_t b = batch ? *batch : q.size(0), h = q.size(1), d = q.size(2);
  const int64_t nblocks = kcache.size(0);
  const int64_t bs = dense ? dense[3] : kcache.size(1);
  const int64_t hkv = kcache.size(dense ? 1 : 2);
  TORCH_CHECK(kcache.size(3) == d, op, ": cache D ", kcache.size(3),
              " != q D ", d);
  TORCH_CHECK(h > 0 && h % hkv == 0, op, ": H % HKV != 0 (", h, ", ", hkv, ")");
  int64_t cs[3] = {bs * hkv * d, hkv * d, d};
  if (dense) {
    const int64_t n = kcache.numel(), cnt[3] = {nblocks, bs, hkv};
    TORCH_CHECK(bs > 0, op, ": block size must be positive, got ", bs);
    // each term of the largest index fits in numel, so their sum cannot wrap
    for (int i = 0; i < 3; ++i) {
      cs[i] = dense[i];
      TORCH_CHECK(cs[i] > 0 && cs[i] % (d / 16) == 0, op,
                  ": cache strides must be positive multiples of ", d / 16,
                  " elements, got ", cs[i]);
      TORCH_CHECK(cnt[i] == 1 || cs[i] <= n / (cnt[i] - 1), op,
                  ": cache strides index past the cache");
    }
    TORCH_CHECK((nblocks - 1) * cs[0] + (bs - 1) * cs[1] + (hkv - 1) * cs[2] +
                    d <= n, op, ": cache strides index past the cache");
  }
  TORCH_CHECK(block_table.is_cuda() && block_table.device() == q.device() &&
              block_table.scalar_type() == torch::kInt &&
              block_table.dim() == 2 && block_table.size(0) == b &&
              block_table.is_contiguous(), op,
              ": block_table must be contiguous int32 [B, max_blocks]");
  TORCH_CHECK(seq_lens.is_cuda() && seq_lens.device() == q.device() &&
              seq_lens.scalar_type() == torch::kInt && seq_lens.dim() == 1 &&
              seq_lens.size(0) == b && seq_lens.is_contiguous(), op,
              ": seq_lens must be contiguous int32 [B]");
  // int32 on the device; the slice rule rounds S up by at most 64 * nsplit
  const int64_t lim = 1LL << 31;
  TORCH_CHECK(nblocks < lim && bs < lim &&
              b * h < (nsplit ? lim / 64 : lim) &&
              block_table.size(1) * bs < (nsplit ? lim - 64 * 64 : lim), op,
              ": size overflow");
  pa::DecodeAttnArgs a{};
  a.q = q.const_data_ptr();
  a.kcache = kcache.const_data_ptr();
  a.vcache = vcache.const_data_ptr();
  a.kscale = int8 ? k_scale->const_data_ptr<float>() : nullptr;
  a.vscale = int8 ? v_scale->const_data_ptr<float>() : nullptr;
  a.block_table = block_table.const_data_ptr<int>();
  a.seq_lens = seq_lens.const_data_ptr<int>();
  a.b = (int)b; a.h = (int)h; a.hkv = (int)hkv; a.bs = (int)bs;
  a.max_blocks = (int)block_table.size(1);
  a.nblocks = (int)nblocks; a.dh = (int)d; a.nsplit = (int)nsplit;
  a.cs_blk = cs[0]; a.cs_pos = cs[1]; a.cs_head = cs[2];
  a.ss_blk = per_token ? bs * hkv : 0;
  a.ss_pos = per_token ? hkv : 0;
  a.ss_head = 1;
  return a;
}

static Tensor launch_paged_decode(pa::DecodeAttnArgs a, const Tensor& q,
                                  double scale) {
  auto o = torch::empty_like(q);
  Tensor o_part, ml_part;
  if (a.nsplit > 0) {
    auto fopt = q.options().dtype(torch::kFloat);
    o_part = torch::empty({a.b, a.h, a.nsplit, a.dh}, fopt);
    ml_part = torch::empty({a.b, a.h, a.nsplit, 2}, fopt);
    a.o_part = o_part.mutable_data_ptr<float>();
    a.ml_part = ml_part.mutable_data_ptr<float>();
  }
  a.o = o.mutable_data_ptr();
  a.scale = (float)scale;
  pa::decode_attention(a, cur_stream());
  return o;
}

// blk_str = pos_str = head_str = bs = 0: paged bf16 caches; else the dense
// layout by the caller's strides (masked_multihead_attention).
Tensor decode_attention(const Tensor& q, const Tensor& kcache,
                        const Tensor& vcache, const Tensor& block_table,
                        const Tensor& seq_lens, double scale, int64_t blk_str,
                        int64_t pos_str, int64_t head_str, int64_t bs) {
  const int64_t dense[4] = {blk_str, pos_str, head_str, bs};
  const bool paged = !blk_str && !pos_str && !head_str && !bs;
  return launch_paged_decode(
      check_paged_decode("decode_attention", q, kcache, vcache, block_table,
                         seq_lens, c10::nullopt, c10::nullopt, 0,
                         paged ? nullptr : dense), q, scale);
}

Tensor decode_attention_int8(const Tensor& q, const Tensor& kcache,
                             const Tensor& vcache, const Tensor& kscale,
                             const Tensor& vscale, const Tensor& block_table,
                             const Tensor& seq_lens, double scale) {
  return launch_paged_decode(
      check_paged_decode("decode_attention_int8", q, kcache, vcache,
                         block_table, seq_lens, kscale, vscale, 0), q, scale);
}

// (gt, tiles, blocks) of the split kernel's grid: the launcher's own plan.
std::tuple<int64_t, int64_t, int64_t> decode_attn_split_grid(
    int64_t b, int64_t h, int64_t hkv, int64_t num_splits, bool int8) {
  TORCH_CHECK(b >= 0 && h > 0 && hkv > 0 && h % hkv == 0 && num_splits >= 1,
              "decode_attn_split_grid: need H % HKV == 0 and num_splits >= 1");
  const pa::DecodeAttnSplitPlan p =
      pa::decode_attn_split_plan(b, h, hkv, num_splits, int8);
  return {p.gt, p.tiles, p.blocks};
}

Tensor decode_attention_split(const Tensor& q, const Tensor& kcache,
                              const Tensor& vcache, const Tensor& block_table,
                              const Tensor& seq_lens, double scale,
                              int64_t num_splits,
                              const c10::optional<Tensor>& k_scale,
                              const c10::optional<Tensor>& v_scale) {
  const char* op = "decode_attention_split";
  TORCH_CHECK(num_splits >= 1 && num_splits <= 64, op,
              ": num_splits must be in [1, 64], got ", num_splits);
  return launch_paged_decode(
      check_paged_decode(op, q, kcache, vcache, block_table, seq_lens, k_scale,
                         v_scale, num_splits), q, scale);
}

// ---- paged prefill attention -------------------------------------------------
// docs/KERNELS.md "paged prefill attention".  Caches, scales and table by
// check_paged_decode; every check precedes any launch or allocation.
Tensor paged_prefill_attention(const Tensor& q, const Tensor& kcache,
                               const Tensor& vcache, const Tensor& block_table,
                               const Tensor& seq_lens, const Tensor& cu_q,
                               int64_t max_q, double scale,
                               const c10::optional<Tensor>& k_scale,
                               const c10::optional<Tensor>& v_scale) {
  const char* op = "paged_prefill_attention";
  TORCH_CHECK(block_table.dim() == 2, op,
              ": block_table must be contiguous int32 [B, max_blocks]");
  const int64_t b = block_table.size(0);
  const pa::DecodeAttnArgs d =
      check_paged_decode(op, q, kcache, vcache, block_table, seq_lens, k_scale,
                         v_scale, 0, nullptr, &b);
  const int64_t t = q.size(0), lim = 1LL << 31;
  TORCH_CHECK(cu_q.is_cuda() && cu_q.device() == q.device() &&
              cu_q.scalar_type() == torch::kInt && cu_q.dim() == 1 &&
              cu_q.size(0) == b + 1 && cu_q.is_contiguous(), op,
              ": cu_q must be contiguous int32 [B + 1]");
  TORCH_CHECK(max_q >= 1 && max_q < lim && max_q * (d.h / d.hkv) < lim, op,
              ": need 1 <= max_q and max_q * H / HKV < 2^31, got ", max_q);
  TORCH_CHECK(t * d.h < lim, op, ": T * H must be below 2^31");
  TORCH_CHECK(b <= 65535 && d.hkv <= 65535, op,
              ": B and HKV must be at most 65535 (grid dimensions)");
  TORCH_CHECK(b >= 1 || t == 0, op, ": tokens without a sequence");
  if (t == 0) return torch::empty_like(q);
  auto o = torch::empty_like(q);
  pa::PrefillAttnArgs a{};
  a.q = d.q; a.kcache = d.kcache; a.vcache = d.vcache;
  a.kscale = d.kscale; a.vscale = d.vscale;
  a.block_table = d.block_table; a.seq_lens = d.seq_lens;
  a.cu_q = cu_q.const_data_ptr<int>();
  a.o = o.mutable_data_ptr();
  a.b = d.b; a.h = d.h; a.hkv = d.hkv; a.bs = d.bs;
  a.max_blocks = d.max_blocks; a.nblocks = d.nblocks; a.dh = d.dh;
  a.t = (int)t; a.max_q = (int)max_q;
  a.scale = (float)scale;
  a.cs_blk = d.cs_blk; a.cs_pos = d.cs_pos; a.cs_head = d.cs_head;
  a.ss_blk = d.ss_blk; a.ss_pos = d.ss_pos; a.ss_head = d.ss_head;
  pa::paged_prefill_attention(a, cur_stream());
  return o;
}

static bool aligned16(const Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.const_data_ptr()) % 16 == 0;
}

// ---- dense MFMA GEMM ---------------------------------------------------------
// Contract of pa::GemmArgs (kernels/api.h, docs/KERNELS.md), shared by
// gemm_bf16_ex, gemm_bf16_nt_batched, gemm_fp8_nt and gemm_fp8_nt_batched:
// both operands are staged by 16-byte accesses through their leading
// dimensions and batch strides, so placement, strides and base alignment are
// checked here, before any launch.  layout: 0=NT 1=NN 2=TN (fp8: NT).
// epilogue: 0=none 1=bias 2=bias_gelu(aux out) 3=dgelu(aux in).  c_in:
// accumulate into it in place (the fused_linear_param_grad_add path).
// Allocates c (and aux for bias_gelu) and fills the args.
struct GemmCall {
  pa::GemmArgs g;
  Tensor c, aux;
};

static GemmCall check_gemm(const char* op, bool fp8, bool batched,
                           const Tensor& a, const Tensor& b, const char* bname,
                           int64_t layout, int64_t epilogue,
                           const c10::optional<Tensor>& bias,
                           const c10::optional<Tensor>& aux_in,
                           const c10::optional<Tensor>& c_in, double scale_ab) {
  const int64_t rank = batched ? 3 : 2;
  const int64_t q = fp8 ? 16 : 8;   // elements per 16 bytes
  const auto bf16 = torch::kBFloat16;
  TORCH_CHECK(a.is_cuda(), op, ": a must be a GPU tensor");
  TORCH_CHECK(b.device() == a.device(), op, ": ", bname, " must be on the device of a");
  if (fp8) {
    auto is_f8 = [](const Tensor& t) {
      return t.scalar_type() == torch::kFloat8_e4m3fn || t.scalar_type() == torch::kUInt8;
    };
    TORCH_CHECK(is_f8(a), op, ": a must be float8_e4m3fn or uint8");
    TORCH_CHECK(is_f8(b), op, ": ", bname, " must be float8_e4m3fn or uint8");
  } else {
    TORCH_CHECK(a.scalar_type() == bf16, op, ": a must be bfloat16");
    TORCH_CHECK(b.scalar_type() == bf16, op, ": ", bname, " must be bfloat16");
  }
  TORCH_CHECK(a.dim() == rank && a.stride(-1) == 1, op, ": a must be ", rank,
              "-D with unit inner stride");
  TORCH_CHECK(b.dim() == rank && b.stride(-1) == 1, op, ": ", bname,
              " must be ", rank, "-D with unit inner stride");
  TORCH_CHECK(layout >= 0 && layout <= 2 && (!fp8 || layout == 0), op,
              ": layout must be 0 (NT), 1 (NN) or 2 (TN), got ", layout);
  TORCH_CHECK(epilogue >= 0 && epilogue <= 3, op,
              ": epilogue must be 0..3, got ", epilogue);
  const bool a_t = layout == pa::kGemmTN, b_t = layout != pa::kGemmNT;
  const int64_t m = a.size(a_t ? -1 : -2), k = a.size(a_t ? -2 : -1);
  const int64_t n = b.size(b_t ? -1 : -2);
  const int64_t batch = batched ? a.size(0) : 1;
  TORCH_CHECK(b.size(b_t ? -2 : -1) == k, op, ": inner dims of a and ", bname,
              " must agree");
  TORCH_CHECK(!batched || b.size(0) == batch, op, ": a and ", bname,
              " must have the same batch size");
  const int64_t kmin = fp8 ? 128 : 64, lim = int64_t(1) << 31;
  TORCH_CHECK(m >= 1 && n >= 1 && m < lim && n < lim && k < lim, op,
              ": 1 <= M, N, K < 2^31, got ", m, ", ", n, ", ", k);
  TORCH_CHECK(k >= kmin, op, ": K must be >= ", kmin, ", got ", k);
  TORCH_CHECK(batch >= 1 && batch <= 65535, op, ": 1 <= batch <= 65535, got ", batch);
  auto strides16 = [&](const Tensor& t) {
    return t.stride(-2) % q == 0 && (!batched || t.stride(0) % q == 0);
  };
  TORCH_CHECK(strides16(a), op, ": a row and batch strides must be multiples of ",
              q, " elements (16 bytes)");
  TORCH_CHECK(strides16(b), op, ": ", bname,
              " row and batch strides must be multiples of ", q, " elements (16 bytes)");
  TORCH_CHECK(aligned16(a), op, ": a data must be 16-byte aligned");
  TORCH_CHECK(aligned16(b), op, ": ", bname, " data must be 16-byte aligned");

  GemmCall call;
  pa::GemmArgs& g = call.g;
  g = pa::GemmArgs{};
  const bool accumulate = c_in.has_value();
  if (accumulate) {
    TORCH_CHECK(epilogue == 0, op, ": accumulate (c_in) requires epilogue 0");
    TORCH_CHECK(c_in->device() == a.device() && c_in->scalar_type() == bf16 &&
                c_in->dim() == 2 && c_in->size(0) == m && c_in->size(1) == n &&
                c_in->stride(1) == 1, op,
                ": c_in must be a bfloat16 [M, N] tensor with unit inner stride "
                "on the device of a");
    call.c = c_in.value();
  } else {
    auto opts = a.options().dtype(bf16);
    call.c = batched ? torch::empty({batch, m, n}, opts) : torch::empty({m, n}, opts);
  }
  const bool reads_bias = fp8 ? bias.has_value() : (epilogue == 1 || epilogue == 2);
  TORCH_CHECK(bias.has_value() == reads_bias, op, ": bias must be given exactly "
              "when the epilogue reads it (epilogue 1 or 2)");
  if (reads_bias) {
    TORCH_CHECK(bias->device() == a.device(), op, ": bias must be on the device of a");
    TORCH_CHECK(bias->scalar_type() == bf16 && bias->is_contiguous(), op,
                ": bias must be contiguous bfloat16");
    if (batched) {
      TORCH_CHECK(bias->dim() == 2 && bias->size(0) == batch && bias->size(1) == n,
                  op, ": bias must be [batch, N]");
    } else {
      TORCH_CHECK(bias->numel() == n, op, ": bias must have N elements");
    }
    g.bias = bias->const_data_ptr();
    g.bias_bs = batched ? n : 0;
  }
  TORCH_CHECK(aux_in.has_value() == (epilogue == 3), op,
              ": aux_in must be given exactly for epilogue 3 (dgelu)");
  if (epilogue == 3) {
    // the kernel walks aux with c's row stride
    TORCH_CHECK(aux_in->device() == a.device() && aux_in->scalar_type() == bf16 &&
                aux_in->dim() == 2 && aux_in->size(0) == m && aux_in->size(1) == n &&
                aux_in->is_contiguous(), op,
                ": aux_in must be a contiguous bfloat16 [M, N] tensor on the device of a");
    g.aux = const_cast<void*>(aux_in->const_data_ptr());
  } else if (epilogue == 2) {
    call.aux = torch::empty({m, n}, a.options());
    g.aux = call.aux.mutable_data_ptr();
  }
  g.a = a.const_data_ptr();
  g.b = b.const_data_ptr();
  g.c = call.c.mutable_data_ptr();
  g.m = m; g.n = n; g.k = k;
  g.lda = a.stride(-2); g.ldb = b.stride(-2); g.ldc = call.c.stride(-2);
  g.batch = batch;
  if (batched) {
    g.a_bs = a.stride(0); g.b_bs = b.stride(0); g.c_bs = call.c.stride(0);
  }
  g.layout = (int)layout;
  g.epilogue = (int)epilogue;
  g.accumulate = accumulate;
  g.scale_ab = (float)scale_ab;
  return call;
}

// Returns {C}, or {C, aux} for bias_gelu.
std::vector<Tensor> gemm_bf16_ex(const Tensor& a, const Tensor& b,
                                 int64_t layout, int64_t epilogue,
                                 const c10::optional<Tensor>& bias,
                                 const c10::optional<Tensor>& aux_in,
                                 const c10::optional<Tensor>& c_in) {
  auto call = check_gemm("gemm_bf16_ex", false, false, a, b, "b", layout,
                         epilogue, bias, aux_in, c_in, 1.0);
  pa::gemm_bf16(call.g, cur_stream());
  if (epilogue == 2) return {call.c, call.aux};
  return {call.c};
}

// Batched NT (grouped experts): C[z] = A[z] @ Bt[z]^T.  The MoE backward is
// the client: dg = dy @ w2^T and dx = dz @ w1^T hit the stored [E, rows, K]
// weight layout directly, dodging both the hipBLASLt strided-transB fault
// (see models/moe.py) and the contiguous weight-transpose workaround.
Tensor gemm_bf16_nt_batched(const Tensor& a, const Tensor& bt) {
  auto call = check_gemm("gemm_bf16_nt_batched", false, true, a, bt, "bt", 0, 0,
                         c10::nullopt, c10::nullopt, c10::nullopt, 1.0);
  pa::gemm_bf16(call.g, cur_stream());
  return call.c;
}

Tensor gemm_fp8_nt(const Tensor& a, const Tensor& bt, double scale_ab,
                   const c10::optional<Tensor>& bias) {
  auto call = check_gemm("gemm_fp8_nt", true, false, a, bt, "bt", 0, 0, bias,
                         c10::nullopt, c10::nullopt, scale_ab);
  pa::gemm_fp8(call.g, cur_stream());
  return call.c;
}

// grouped/batched variant: one launch over all experts, bias [E, N]
Tensor gemm_fp8_nt_batched(const Tensor& a, const Tensor& bt, double scale_ab,
                           const c10::optional<Tensor>& bias) {
  auto call = check_gemm("gemm_fp8_nt_batched", true, true, a, bt, "bt", 0, 0,
                         bias, c10::nullopt, c10::nullopt, scale_ab);
  pa::gemm_fp8(call.g, cur_stream());
  return call.c;
}

// Contract of the MFMA W-streamer (decode_stream_kernel, docs/KERNELS.md),
// shared by decode_gemm_mfma / _int8 / _int4: every lane does 16-byte loads
// of whole 64 x 256 weight tiles and of x rows, so shapes, placement and base
// alignment are checked here, before any launch.  The callers check what is
// specific to their weight format first; `k` is the K their weight holds,
// `kdesc` names it in the message.  Allocates the split-K workspace and y.
struct DecodeStreamCall {
  int64_t m, n, k;
  const void* bias;
  Tensor ws, y;
};

static DecodeStreamCall check_decode_stream(const char* op, const Tensor& x,
                                            const Tensor& w, int64_t k,
                                            const char* kdesc,
                                            const c10::optional<Tensor>& bias,
                                            int64_t ksplit) {
  CHECK_IN(x);
  TORCH_CHECK(x.dim() == 2 && x.scalar_type() == torch::kBFloat16, op,
              ": x must be a 2-D bf16 tensor");
  TORCH_CHECK(w.device() == x.device(), op, ": weight and x must be on one device");
  const int64_t m = x.size(0), n = w.size(1);
  TORCH_CHECK(x.size(1) == k, op, ": ", kdesc, " must equal K");
  TORCH_CHECK(m >= 1 && m <= 32, op, ": 1 <= M <= 32, got ", m);
  TORCH_CHECK(n > 0 && n % 256 == 0, op, ": N % 256 == 0, got ", n);
  TORCH_CHECK(k > 0 && k % 64 == 0 && k <= (int64_t(1) << 24), op,
              ": K % 64 == 0 (and K <= 2^24), got ", k);
  TORCH_CHECK(aligned16(x) && aligned16(w), op,
              ": x and weight data must be 16-byte aligned");
  TORCH_CHECK(ksplit >= 0, op, ": ksplit >= 0");
  const void* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() &&
                bias->scalar_type() == torch::kBFloat16 && bias->numel() == n,
                op, ": bias must be contiguous bf16 with N elements");
    bp = bias->const_data_ptr();
  }
  const int64_t splits = pa::decode_split_plan(k, n, ksplit).splits;
  const int64_t mt = m <= 16 ? 16 : 32;
  return {m, n, k, bp,
          torch::empty({splits, mt, n}, x.options().dtype(torch::kFloat)),
          torch::empty({m, n}, x.options())};
}

Tensor decode_gemm_mfma(const Tensor& x, const Tensor& w,
                        const c10::optional<Tensor>& bias) {
  const char* op = "decode_gemm_mfma";
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.scalar_type() == torch::kBFloat16,
              op, ": w must be a 2-D bf16 GPU tensor");
  TORCH_CHECK(w.stride(1) == 1 && w.stride(0) % 8 == 0, op,
              ": w must have unit column stride and a row stride % 8 == 0");
  auto c = check_decode_stream(op, x, w, w.size(0), "w.size(0)", bias, 0);
  pa::decode_gemm_mfma(x.const_data_ptr(), w.const_data_ptr(), c.bias,
                       c.y.mutable_data_ptr(), c.ws.mutable_data_ptr<float>(),
                       c.m, c.n, c.k, w.stride(0), 0, cur_stream());
  return c.y;
}

// qw int8 [K, N] contiguous, scale fp32 [N] (weight_quantize, int8)
Tensor decode_gemm_int8(const Tensor& x, const Tensor& qw,
                        const Tensor& scale,
                        const c10::optional<Tensor>& bias) {
  const char* op = "decode_gemm_int8";
  TORCH_CHECK(qw.is_cuda() && scale.is_cuda(), op, ": qw and scale must be GPU tensors");
  TORCH_CHECK(qw.dim() == 2 && qw.is_contiguous(), op,
              ": qw must be a contiguous [K, N] tensor");
  TORCH_CHECK(qw.scalar_type() == torch::kChar, op, ": qw must be int8");
  TORCH_CHECK(scale.scalar_type() == torch::kFloat && scale.is_contiguous(),
              op, ": scale must be contiguous fp32");
  TORCH_CHECK(scale.dim() == 1 && scale.size(0) == qw.size(1), op,
              ": per-channel scale must be [N]");
  auto c = check_decode_stream(op, x, qw, qw.size(0), "qw.size(0)", bias, 0);
  pa::decode_gemm_int8(x.const_data_ptr(), qw.const_data_ptr(),
                       scale.const_data_ptr<float>(), c.bias,
                       c.y.mutable_data_ptr(), c.ws.mutable_data_ptr<float>(),
                       c.m, c.n, c.k, 0, cur_stream());
  return c.y;
}

// int4 weight-only storage shared by decode_gemm_int4 and dequant_int4:
// qw int8 [K/2, N] contiguous (two codes per byte), scale fp32 [N]
// (group_size -1) or [K/group_size, N] (group_size 64 | 128).  Returns K.
static int64_t check_int4_weight(const Tensor& qw, const Tensor& scale,
                                 int64_t group_size, const char* op) {
  TORCH_CHECK(qw.is_cuda() && scale.is_cuda(), op, ": qw and scale must be GPU tensors");
  TORCH_CHECK(qw.dim() == 2 && qw.is_contiguous(), op,
              ": qw must be a contiguous [K/2, N] tensor");
  TORCH_CHECK(qw.scalar_type() == torch::kChar, op, ": qw must be int8");
  TORCH_CHECK(scale.scalar_type() == torch::kFloat && scale.is_contiguous(),
              op, ": scale must be contiguous fp32");
  TORCH_CHECK(group_size == -1 || group_size == 64 || group_size == 128, op,
              ": group_size must be -1, 64 or 128, got ", group_size);
  const int64_t k = qw.size(0) * 2, n = qw.size(1);
  if (group_size == -1) {
    TORCH_CHECK(scale.dim() == 1 && scale.size(0) == n, op,
                ": per-channel scale must be [N]");
  } else {
    TORCH_CHECK(k % group_size == 0, op, ": K must be a multiple of group_size");
    TORCH_CHECK(scale.dim() == 2 && scale.size(0) == k / group_size &&
                scale.size(1) == n, op, ": group scale must be [K/group_size, N]");
  }
  return k;
}

Tensor decode_gemm_int4(const Tensor& x, const Tensor& qw, const Tensor& scale,
                        const c10::optional<Tensor>& bias, int64_t group_size,
                        int64_t ksplit) {
  const char* op = "decode_gemm_int4";
  const int64_t k = check_int4_weight(qw, scale, group_size, op);
  auto c = check_decode_stream(op, x, qw, k, "qw.size(0)*2", bias, ksplit);
  pa::decode_gemm_int4(x.const_data_ptr(), qw.const_data_ptr(),
                       scale.const_data_ptr<float>(), c.bias,
                       c.y.mutable_data_ptr(), c.ws.mutable_data_ptr<float>(),
                       c.m, c.n, c.k, group_size, ksplit, cur_stream());
  return c.y;
}

Tensor dequant_int4(const Tensor& qw, const Tensor& scale, int64_t group_size,
                    at::ScalarType out_dtype) {
  const int64_t k = check_int4_weight(qw, scale, group_size, "dequant_int4");
  const int64_t n = qw.size(1);
  TORCH_CHECK(n % 8 == 0, "dequant_int4: N % 8 == 0, got ", n);
  TORCH_CHECK(out_dtype == torch::kBFloat16 || out_dtype == torch::kFloat,
              "dequant_int4: out_dtype must be bfloat16 or float32");
  auto out = torch::empty({k, n}, qw.options().dtype(out_dtype));
  pa::dequant_int4(qw.const_data_ptr(), scale.const_data_ptr<float>(),
                   out.mutable_data_ptr(), k, n, group_size,
                   out_dtype == torch::kBFloat16 ? pa::kBF16 : pa::kF32,
                   cur_stream());
  return out;
}

// ---- MoE routing ----------------------------------------------------------
std::vector<Tensor> moe_gate_topk(const Tensor& logits, int64_t k) {
  CHECK_IN(logits);
  TORCH_CHECK(logits.scalar_type() == torch::kFloat && logits.dim() == 2);
  int64_t t = logits.size(0), e = logits.size(1);
  TORCH_CHECK(e <= 64 && k <= 4);
  auto topv = torch::empty({t, k}, logits.options());
  auto topi = torch::empty({t, k}, logits.options().dtype(torch::kInt32));
  auto me = torch::zeros({e}, logits.options());
  auto ce = torch::zeros({e}, logits.options());
  pa::moe_gate_topk(logits.const_data_ptr<float>(), topv.mutable_data_ptr<float>(),
                    topi.mutable_data_ptr<int>(), me.mutable_data_ptr<float>(),
                    ce.mutable_data_ptr<float>(), t, e, k, cur_stream());
  return {topv, topi, me, ce};
}

std::vector<Tensor> moe_assign_slots(const Tensor& topi, int64_t num_experts,
                                     int64_t cap) {
  CHECK_IN(topi);
  TORCH_CHECK(topi.scalar_type() == torch::kInt32 && topi.dim() == 2);
  int64_t t = topi.size(0), k = topi.size(1);
  auto slot = torch::full({t, k}, -1, topi.options());
  auto counts = torch::zeros({num_experts}, topi.options());
  pa::moe_assign_slots(topi.const_data_ptr<int>(), slot.mutable_data_ptr<int>(),
                       counts.mutable_data_ptr<int>(), t, num_experts, k, cap,
                       cur_stream());
  return {slot, counts};
}

Tensor amax_abs(const Tensor& x) {
  CHECK_IN(x);
  auto out = torch::zeros({}, x.options().dtype(torch::kFloat));
  pa::amax_abs(x.const_data_ptr(), out.mutable_data_ptr<float>(), x.numel(),
               dt_of(x), cur_stream());
  return out;
}

Tensor quant_fp8(const Tensor& x, double scale) {
  CHECK_IN(x);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.numel() % 8 == 0);
  auto out = torch::empty(x.sizes(), x.options().dtype(torch::kFloat8_e4m3fn));
  pa::quant_fp8(x.const_data_ptr(), out.mutable_data_ptr(), (float)scale,
                x.numel(), cur_stream());
  return out;
}

// ---- probe ----------------------------------------------------------------
Tensor mfma_probe_fp8mx(const Tensor& a, const Tensor& bt, int64_t sa, int64_t sb) {
  CHECK_IN(a); CHECK_IN(bt);
  TORCH_CHECK(a.scalar_type() == torch::kUInt8 && a.numel() == 16 * 128);
  auto c = torch::empty({16, 16}, a.options().dtype(torch::kFloat));
  pa::mfma_probe_fp8mx(a.const_data_ptr(), bt.const_data_ptr(),
                       c.mutable_data_ptr<float>(), (int)sa, (int)sb,
                       cur_stream());
  return c;
}

Tensor mfma_probe(const Tensor& a, const Tensor& bt) {
  CHECK_IN(a); CHECK_IN(bt);
  auto c = torch::empty({16, 16}, a.options().dtype(torch::kFloat));
  pa::mfma_probe(a.const_data_ptr(), bt.const_data_ptr(),
                 c.mutable_data_ptr<float>(), cur_stream());
  return c;
}

Tensor mfma_probe32(const Tensor& a, const Tensor& bt) {
  CHECK_IN(a); CHECK_IN(bt);
  auto c = torch::empty({32, 32}, a.options().dtype(torch::kFloat));
  pa::mfma_probe32(a.const_data_ptr(), bt.const_data_ptr(),
                   c.mutable_data_ptr<float>(), cur_stream());
  return c;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("layer_norm_fwd", &layer_norm_fwd);
  m.def("layer_norm_bwd", &layer_norm_bwd, py::arg("dy"), py::arg("x"),
        py::arg("w"), py::arg("mean"), py::arg("rstd"), py::arg("has_bias"),
        py::arg("dres") = c10::nullopt, py::arg("fused") = true,
        py::arg("grid_cap") = 0);
  m.def("add_layer_norm_fwd", &add_layer_norm_fwd, py::arg("x"),
        py::arg("residual"), py::arg("w"), py::arg("b") = c10::nullopt,
        py::arg("eps") = 1e-5);
  m.def("ln_bwd_grid_cap", &ln_bwd_grid_cap);
  m.def("ln_fused_ok", &ln_fused_ok);
  m.def("bias_gelu_bwd_db", &bias_gelu_bwd_db, py::arg("dy"), py::arg("x"),
        py::arg("bias") = c10::nullopt, py::arg("fused") = true);
  m.def("bias_gelu_bwd_db_fused", &bias_gelu_bwd_db_fused);
  m.def("flash_attn_bwd_delta", &flash_attn_bwd_delta);
  m.def("rms_norm_fwd", &rms_norm_fwd);
  m.def("rms_norm_bwd", &rms_norm_bwd);
  m.def("softmax_ce_fwd", &softmax_ce_fwd);
  m.def("softmax_ce_bwd", &softmax_ce_bwd);
  m.def("bias_gelu_fwd", &bias_gelu_fwd);
  m.def("bias_gelu_bwd", &bias_gelu_bwd);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("rope_fwd", &rope_fwd);
  m.def("colsum", &colsum);
  m.def("adamw", &adamw);
  m.def("fc1_gelu_fwd", &pa_lt::fc1_gelu_fwd);
  m.def("fc2_dgrad_dgelu", &pa_lt::fc2_dgrad_dgelu);
  m.def("lt_epilogue_probe", &pa_lt::lt_epilogue_probe);
  m.def("l2norm_sq", &l2norm_sq);
  m.def("flash_attn_fwd", &flash_attn_fwd, py::arg("q"), py::arg("k"),
        py::arg("v"), py::arg("o") = c10::nullopt, py::arg("scale"),
        py::arg("causal"), py::arg("mask") = c10::nullopt,
        py::arg("pdrop") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0);
  m.def("fa_dropout_mask", &fa_dropout_mask);
  m.def("mfma_probe_fp8mx", &mfma_probe_fp8mx);
  m.def("decode_gemm_mfma", &decode_gemm_mfma, py::arg("x"), py::arg("w"),
        py::arg("bias") = c10::nullopt);
  m.def("decode_gemm_int8", &decode_gemm_int8, py::arg("x"), py::arg("qw"),
        py::arg("scale"), py::arg("bias") = c10::nullopt);
  m.def("decode_gemm_int4", &decode_gemm_int4, py::arg("x"), py::arg("qw"),
        py::arg("scale"), py::arg("bias") = c10::nullopt,
        py::arg("group_size") = -1, py::arg("ksplit") = 0);
  m.def("dequant_int4", &dequant_int4, py::arg("qw"), py::arg("scale"),
        py::arg("group_size"), py::arg("out_dtype"));
  m.def("moe_gate_topk", &moe_gate_topk);
  m.def("moe_assign_slots", &moe_assign_slots);
  m.def("gemm_fp8_nt", &gemm_fp8_nt, py::arg("a"), py::arg("bt"),
        py::arg("scale_ab") = 1.0, py::arg("bias") = c10::nullopt);
  m.def("gemm_fp8_nt_batched", &gemm_fp8_nt_batched, py::arg("a"),
        py::arg("bt"), py::arg("scale_ab"), py::arg("bias") = c10::nullopt);
  m.def("amax_abs", &amax_abs);
  m.def("quant_fp8", &quant_fp8);
  m.def("flash_attn_varlen_fwd", &flash_attn_varlen_fwd, py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("cu_q"), py::arg("cu_k"),
        py::arg("scale"), py::arg("causal"), py::arg("pdrop") = 0.0,
        py::arg("seed") = 0, py::arg("offset") = 0);
  m.def("flash_attn_varlen_bwd", &flash_attn_varlen_bwd, py::arg("dout"),
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"), py::arg("lse"),
        py::arg("cu_q"), py::arg("cu_k"), py::arg("scale"), py::arg("causal"),
        py::arg("pdrop"), py::arg("seed"), py::arg("offset"),
        py::arg("gqa_heads_per_block") = 0);
  m.def("flash_attn_bwd", &flash_attn_bwd, py::arg("dout"), py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("o"), py::arg("lse"),
        py::arg("dq") = c10::nullopt, py::arg("dk") = c10::nullopt,
        py::arg("dv") = c10::nullopt, py::arg("scale"), py::arg("causal"),
        py::arg("mask") = c10::nullopt, py::arg("pdrop") = 0.0,
        py::arg("seed") = 0, py::arg("offset") = 0,
        py::arg("gqa_heads_per_block") = 0);
  m.def("dropout_add_fwd", &dropout_add_fwd);
  m.def("dropout_add_bwd", &dropout_add_bwd);
  m.def("embedding_fwd", &embedding_fwd);
  m.def("embedding_bwd", &embedding_bwd);
  m.def("gemm_bf16_nt_batched", &gemm_bf16_nt_batched);
  m.def("gemm_bf16_ex", &gemm_bf16_ex, py::arg("a"), py::arg("b"),
        py::arg("layout"), py::arg("epilogue") = 0,
        py::arg("bias") = c10::nullopt, py::arg("aux") = c10::nullopt,
        py::arg("c_in") = c10::nullopt);
  m.def("decode_attention", &decode_attention, py::arg("q"), py::arg("kcache"),
        py::arg("vcache"), py::arg("block_table"), py::arg("seq_lens"),
        py::arg("scale"), py::arg("blk_str") = 0, py::arg("pos_str") = 0,
        py::arg("head_str") = 0, py::arg("bs_override") = 0);
  m.def("kv_quant_append", &kv_quant_append, py::arg("k"), py::arg("v"),
        py::arg("kcache"), py::arg("vcache"), py::arg("kscale"),
        py::arg("vscale"), py::arg("blk"), py::arg("off"),
        py::arg("k_qscale") = c10::nullopt, py::arg("v_qscale") = c10::nullopt);
  m.def("decode_attention_int8", &decode_attention_int8, py::arg("q"),
        py::arg("kcache"), py::arg("vcache"), py::arg("kscale"),
        py::arg("vscale"), py::arg("block_table"), py::arg("seq_lens"),
        py::arg("scale"));
  m.def("decode_attention_split", &decode_attention_split, py::arg("q"),
        py::arg("kcache"), py::arg("vcache"), py::arg("block_table"),
        py::arg("seq_lens"), py::arg("scale"), py::arg("num_splits"),
        py::arg("k_scale") = c10::nullopt, py::arg("v_scale") = c10::nullopt);
  m.def("paged_prefill_attention", &paged_prefill_attention, py::arg("q"),
        py::arg("kcache"), py::arg("vcache"), py::arg("block_table"),
        py::arg("seq_lens"), py::arg("cu_q"), py::arg("max_q"),
        py::arg("scale"), py::arg("k_scale") = c10::nullopt,
        py::arg("v_scale") = c10::nullopt);
  m.def("decode_attn_split_grid", &decode_attn_split_grid, py::arg("b"),
        py::arg("h"), py::arg("hkv"), py::arg("num_splits"), py::arg("int8"));
  m.def("mfma_probe", &mfma_probe);
  m.def("mfma_probe32", &mfma_probe32);
  m.attr("compiled_arch") = "gfx950";
}
