// C ABI between the torch binding layer (bindings.cpp, compiled by g++)
// and the gfx950 kernel library (*.hip, compiled by hipcc).
// Raw pointers + hipStream_t only -- no torch types cross this line.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pa {

// dtype tags for the few we support natively
enum DType : int { kBF16 = 0, kF32 = 1, kF16 = 2 };

// ---- norms ----------------------------------------------------------------
void layer_norm_fwd(const void* x, const void* w, const void* b, void* y,
                    float* mean, float* rstd, int64_t n, int64_t d, float eps,
                    int dtype, hipStream_t s);
void layer_norm_bwd_dx(const void* dy, const void* x, const void* w,
                       const float* mean, const float* rstd, void* dx,
                       int64_t n, int64_t d, int dtype, hipStream_t s);
// dw / db of the two-kernel backward, d % 8 == 0.  One column walk writes
// per-chunk partials to ws, fp32 [col_chunks(n, d)][nout][d] with nout = 2
// (layer_norm_bwd_dwdb: dw and db, db may be null) or 1 (rms_norm_bwd_dw), and
// ws_reduce adds them in a fixed order: ws and the outputs need no
// initialisation.  col_chunks is also the row-chunk count of colsum's grid.
int col_chunks(int64_t n, int64_t d);
void layer_norm_bwd_dwdb(const void* dy, const void* x, const float* mean,
                         const float* rstd, float* dw, float* db, float* ws,
                         int64_t n, int64_t d, int dtype, hipStream_t s);
void rms_norm_bwd_dw(const void* dy, const void* x, const float* rstd,
                     float* dw, float* ws, int64_t n, int64_t d, int dtype,
                     hipStream_t s);

// Register-resident fused norms (d % 8 == 0, d <= kLnFusedMaxD).
constexpr int64_t kLnFusedMaxD = 8192;
// row-block cap of the one-pass backward (measured, docs/KERNELS.md)
constexpr int kLnBwdGridCap = 1024;
bool ln_fused_ok(int64_t d);
int ln_bwd_fused_grid(int64_t n, int cap);  // cap <= 0: kLnBwdGridCap
// h = x + residual (stored), y = LN(h); bit-equal to dropout_add_fwd(p=0)
// followed by layer_norm_fwd
void add_layer_norm_fwd(const void* x, const void* residual, const void* w,
                        const void* b, void* h, void* y, float* mean,
                        float* rstd, int64_t n, int64_t d, float eps, int dtype,
                        hipStream_t s);
// dx (+ dres, may be null), dw and db (may be null) from one read of dy and
// x.  ws: fp32 [grid, 2, d] partials, grid = ln_bwd_fused_grid(n, cap).
void layer_norm_bwd_fused(const void* dy, const void* x, const void* w,
                          const float* mean, const float* rstd,
                          const void* dres, void* dx, float* dw, float* db,
                          float* ws, int grid, int64_t n, int64_t d, int dtype,
                          hipStream_t s);
// out0[d] (and out1[d], may be null) = sum over parts of ws[parts][nout][d]
void ws_reduce(const float* ws, float* out0, float* out1, int parts, int nout,
               int64_t d, hipStream_t s);

void rms_norm_fwd(const void* x, const void* residual, const void* w, void* y,
                  void* res_out, float* rstd, int64_t n, int64_t d, float eps,
                  int dtype, hipStream_t s);
void rms_norm_bwd_dx(const void* dy, const void* x, const void* w,
                     const float* rstd, void* dx, int64_t n, int64_t d,
                     int dtype, hipStream_t s);

// ---- fused softmax cross-entropy ------------------------------------------
// logits [n, v]; labels int64 [n]; loss/lse fp32 [n]
void softmax_ce_fwd(const void* logits, const int64_t* labels, float* loss,
                    float* lse, int64_t n, int64_t v, int64_t ignore_index,
                    int dtype, hipStream_t s);
// dlogits written in logits dtype; dloss fp32 [n]
void softmax_ce_bwd(const float* dloss, const void* logits,
                    const int64_t* labels, const float* lse, void* dlogits,
                    int64_t n, int64_t v, int64_t ignore_index, int dtype,
                    hipStream_t s);

// ---- elementwise fusions ---------------------------------------------------
// y = gelu(x + bias); bias [d] may be null
void bias_gelu_fwd(const void* x, const void* bias, void* y, int64_t n,
                   int64_t d, int dtype, hipStream_t s);
// dx = gelu'(x+bias) * dy  (the bias gradient: bias_gelu_bwd_db, or colsum of dx)
void bias_gelu_bwd(const void* dy, const void* x, const void* bias, void* dx,
                   int64_t n, int64_t d, int dtype, hipStream_t s);
// Same dx, plus db[d] = colsum(dx as stored) from per-thread partials.
// grid = bias_gelu_bwd_db_grid(n, d); 0 means no grid keeps a thread on the
// same columns and the caller runs bias_gelu_bwd + colsum.  ws: fp32
// [grid * 256 * W] with W = 16 if d % 16 == 0 else 8.
int bias_gelu_bwd_db_grid(int64_t n, int64_t d);
void bias_gelu_bwd_db(const void* dy, const void* x, const void* bias, void* dx,
                      float* db, float* ws, int grid, int64_t n, int64_t d,
                      int dtype, hipStream_t s);

// swiglu: x [n, 2d] = [gate | up]; y [n, d] = silu(gate) * up
void swiglu_fwd(const void* x, void* y, int64_t n, int64_t d, int dtype,
                hipStream_t s);
void swiglu_bwd(const void* dy, const void* x, void* dx, int64_t n, int64_t d,
                int dtype, hipStream_t s);

// rope (neox rotate-half): qk [b, s, h, dh], cos/sin fp32 [s, dh/2]
// backward == forward with conj=true (sin negated)
void rope_fwd(const void* x, const float* cos_t, const float* sin_t, void* y,
              int64_t b, int64_t sl, int64_t h, int64_t dh, int64_t pos_offset,
              bool conj, int dtype, hipStream_t s);

// out[0] = max |x| over a flat buffer (atomic max into a zeroed fp32)
void amax_abs(const void* x, float* out, int64_t n, int dtype, hipStream_t s);
// column-sum of [n, d], any d, added into a zeroed fp32 [d] by atomics (bias
// grads): the last bits depend on dispatch order
void colsum(const void* x, float* out, int64_t n, int64_t d, int dtype,
            hipStream_t s);

// ---- transpose with column sums (transpose.hip) -----------------------------
// out [c, r] contiguous = x [r, c]^T, bf16, x with unit inner stride and row
// stride ld in elements.  sums non-null: sums[c] = fp32 column sums of x, from
// per-chunk partials ws [transpose_plan(r, c).chunks][c] added in a fixed
// order (ws and sums need no initialisation, no atomics).
// Contract (checked by the binding): r % 8 == 0, c % 8 == 0, ld % 8 == 0,
// 1 <= r, c < 2^31, x and out 16-byte aligned.
struct TransposePlan { int tiles_per_chunk, chunks; };
TransposePlan transpose_plan(int64_t r, int64_t c);
void transpose_colsum(const void* x, void* out, float* sums, float* ws,
                      int64_t r, int64_t c, int64_t ld, hipStream_t s);

// ---- fused AdamW (flat shards; fp32 master + bf16 model params) -----------
void adamw(float* master, void* param_bf16, const void* grad, float* m,
           float* v, int64_t numel, float lr, float beta1, float beta2,
           float eps, float wd, float beta1_pow, float beta2_pow,
           float grad_scale, int grad_dtype, bool param_out_bf16, hipStream_t s);

// multi-tensor l2-norm^2 of a flat fp32/bf16 buffer -> out[0] (fp32, add)
void l2norm_sq(const void* x, float* out, int64_t numel, int dtype,
               hipStream_t s);

// ---- flash attention (bf16, head_dim 128 or 64) ----------------------------
// Dense: logical layout [b, h, s, dh] with per-tensor (batch, head, seq)
// ELEMENT strides (dh innermost and contiguous, 16-byte aligned rows), so
// packed [b, s, 3, h, dh] qkv views need no transpose copies.  v shares k's
// strides, dv shares dk's.  lse / delta fp32 [b, h, sq] contiguous.
// mask: additive bf16 [b|1, h|1, sq, skv] by m_s (0 = broadcast), null =
// none.  pdrop > 0 with (seed, offset): Philox attention dropout, the same
// keep mask in forward and backward (fa_dropout_mask materialises it).
// Varlen (cu_q != null): packed [total, h, dh] tensors, b = 1, sq / skv the
// packed totals, strides {0, dh, h * dh}; cu_q / cu_k int32 [nseq + 1] prefix
// sums; q_bmap / kv_bmap int32 (seq, row-within-seq) pairs, one per 128-row
// block; lse / delta [h, total_q]; causal is bottom-right aligned; no mask.
// GQA: h a multiple of hkv, q head i reads K/V head i / (h / hkv); k, v, dk
// and dv have hkv heads.  The backward takes hkv != h without a mask only.
// gqa_heads: q heads per dK/dV block, a divisor of h / hkv, 0 = the whole
// group; below h / hkv the blocks write fp32 partials to gqa_ws, 2 * b *
// (h / gqa_heads) * skv * dh floats (dK, then dV), which a reduce kernel sums.
// FlashMask (fm_bounds != null; flashmask.hip): per key column up to two
// half-open ranges of query rows that may not see it, on top of causal.
// flashmask_prep writes both tensors from startend_row_indices: fm_bounds
// int32 [b, fm_hm, 4, skv8] (lo0 | hi0 | lo1 | hi1, skv8 = skv rounded up to
// 8), fm_tiles int32 [b, fm_hm, ceil(skv / 64), 8] (per 64-column tile and
// range: max lo, min hi, min lo, max hi).  fm_hm is 1 or hkv (the mask head
// of q head i is its kv head), fm_nr the ranges the form can fill (1 or 2).
// Dense only, no additive mask, no dropout; the backward takes hkv == h.
struct FaStride { long long b, h, s; };
struct FaArgs {
  const void *q, *k, *v;
  void* o;              // forward: written; backward: read
  const void* dout;
  void *dq, *dk, *dv;
  float* lse;           // forward: written; backward: read
  float* delta;         // backward workspace, shaped like lse
  const void* mask;
  int b, h, hkv, sq, skv, dh;
  float scale;
  bool causal;
  FaStride q_s, k_s, o_s, do_s, dq_s, dk_s, m_s;
  float pdrop;
  unsigned long long seed, offset;
  const int *cu_q, *cu_k, *q_bmap, *kv_bmap;
  int n_qblocks, n_kvblocks;
  int gqa_heads;        // backward
  float* gqa_ws;        // backward workspace, null unless gqa_heads < h / hkv
  const int *fm_bounds, *fm_tiles;   // FlashMask, null = none
  int fm_hm, fm_nr;
};
// startend_row_indices int32 [b_hm, skv, c] -> bounds, tiles (see above); one
// launch, no atomics, no host read, every output element written
void flashmask_prep(const int* idx, int* bounds, int* tiles, int64_t b_hm, int64_t sq,
                    int64_t skv, int c, bool causal, hipStream_t s);
// what flash_attn_fwd / flash_attn_bwd (after delta) launch with fm_bounds set
void flashmask_attn_fwd(const FaArgs& a, hipStream_t s);
void flashmask_attn_bwd(const FaArgs& a, hipStream_t s);
void flash_attn_fwd(const FaArgs& a, hipStream_t s);
// delta = rowsum(dout * o), then dK / dV and dQ
void flash_attn_bwd(const FaArgs& a, hipStream_t s);
// delta[b, h, sq] = rowsum(dout * o) alone: the first kernel of the backward
void flash_attn_bwd_delta(const void* dout, const void* o, float* delta,
                          int64_t b, int64_t h, int64_t sq, int64_t dh,
                          const FaStride& dos, const FaStride& os, hipStream_t s);
// materialize the dropout keep-mask (debug/tests): out uint8 [total]
void fa_dropout_mask(void* out, int64_t total, float p, uint64_t seed,
                     uint64_t offset, hipStream_t s);

// ---- dropout + residual add ------------------------------------------------
// y = dropout(x, p) + residual; mask stored as uint8 per element
void dropout_add_fwd(const void* x, const void* residual, void* y,
                     uint8_t* mask, int64_t numel, float p, uint64_t seed,
                     uint64_t offset, int dtype, hipStream_t s);
void dropout_add_bwd(const void* dy, const uint8_t* mask, void* dx,
                     int64_t numel, float p, int dtype, hipStream_t s);

// ---- embedding -------------------------------------------------------------
void embedding_fwd(const void* table, const int64_t* ids, void* out,
                   int64_t n_ids, int64_t d, int64_t vocab, int64_t padding_idx,
                   int dtype, hipStream_t s);
// grad table accumulated fp32 (atomics)
void embedding_bwd(const void* dout, const int64_t* ids, float* dtable,
                   int64_t n_ids, int64_t d, int64_t vocab, int64_t padding_idx,
                   int dtype, hipStream_t s);

// ---- int8 paged KV cache: quantize-on-append --------------------------------
// codes int8 [nblocks, bs, HKV, D]; scales fp32 addressed (blk, pos, head)
// by element strides: per token [nblocks, bs, HKV] -> (bs*HKV, HKV, 1), per
// head [HKV] -> (0, 0, 1).
// kv_quant_append: k/v bf16 [T, HKV, D] by token/head strides in elements
// (D contiguous, 16-byte aligned rows).  k_qscale/v_qscale null: per-token
// mode, writes d = absmax * fp32(1/127) into kscale/vscale; else fixed mode,
// code = rint(x * qscale[h]) and the scale pools are not touched.
void kv_quant_append(const void* k, const void* v, void* kcache, void* vcache,
                     float* kscale, float* vscale, const int64_t* blk,
                     const int64_t* off, const float* k_qscale,
                     const float* v_qscale, int64_t t, int64_t hkv, int64_t dh,
                     int64_t bs, int64_t nblocks, int64_t k_tstr,
                     int64_t k_hstr, int64_t v_tstr, int64_t v_hstr,
                     hipStream_t s);

// ---- paged decode attention (decode_attn.hip) ------------------------------
// One kernel for every path.  A block owns (split, head tile, kv head,
// sequence): a tile of `gt` consecutive q-heads of one kv head's group
// G = H/HKV shares each K/V load, `tiles` = ceil(G / gt) tiles per kv head.
// Split launches (nsplit >= 1) take gt and the grid from
// decode_attn_split_plan: gt is the smallest instantiated tile >= G, at most
// 8 (bf16 cache) or 4 (int8 cache), grid = b * hkv * tiles * nsplit blocks.
// Unsplit launches (nsplit == 0) use gt = 1, one block per (b, q-head).
struct DecodeAttnSplitPlan { int gt, tiles; int64_t blocks; };
DecodeAttnSplitPlan decode_attn_split_plan(int64_t b, int64_t h, int64_t hkv,
                                           int64_t nsplit, bool int8);
// q, o bf16 [b, h, dh] contiguous; block_table int32 [b, max_blocks];
// seq_lens int32 [b].  kscale/vscale null: bf16 cache; else int8 codes with
// fp32 scales.  Codes and scales are addressed (blk, pos, head) by element
// strides cs_* / ss_*; a table entry outside [0, nblocks) reads nothing.
// S_b = max(0, min(seq_lens[b], max_blocks * bs)).
// nsplit == 0: one pass over [0, S_b) writes o; no workspace.
// 1 <= nsplit <= 64: slice rule on the device, c_b = 64 * ceil(S_b / (64 *
// nsplit)), split s covers [s * c_b, min(S_b, (s + 1) * c_b)); fp32
// workspaces o_part [b, h, nsplit, dh] (unnormalised, relative to the
// split's max) and ml_part [b, h, nsplit, 2] (max, sum) are written in full
// by the first kernel before the merge kernel reads them.
struct DecodeAttnArgs {
  const void *q, *kcache, *vcache;
  const float *kscale, *vscale;
  const int *block_table, *seq_lens;
  void* o;
  float *o_part, *ml_part;
  int b, h, hkv, bs, max_blocks, nblocks, dh, nsplit;
  float scale;
  long long cs_blk, cs_pos, cs_head;
  long long ss_blk, ss_pos, ss_head;
};
void decode_attention(const DecodeAttnArgs& a, hipStream_t s);

// ---- paged prefill attention (prefill_attn.hip) ----------------------------
// q_len_b = cu_q[b+1] - cu_q[b] >= 1 new tokens per sequence attend to the
// paged cache.  q, o bf16 [t, h, dh] packed over sequences; cu_q int32
// [b + 1]; caches, scales, table and their cs_* / ss_* strides as in
// DecodeAttnArgs (paged layout only).  seq_lens[b] counts the new tokens;
// S_b = max(0, min(seq_lens[b], max_blocks * bs)); token i of sequence b
// sits at position S_b - q_len_b + i and sees positions 0 .. that one.
// Grid (ceil(max_q * h / hkv / 64), hkv, b): rows of a sequence with
// q_len_b > max_q past the grid are not computed.  No workspace, no atomics,
// no host read.
struct PrefillAttnArgs {
  const void *q, *kcache, *vcache;
  const float *kscale, *vscale;
  const int *block_table, *seq_lens, *cu_q;
  void* o;
  int b, h, hkv, bs, max_blocks, nblocks, dh, t, max_q;
  float scale;
  long long cs_blk, cs_pos, cs_head;
  long long ss_blk, ss_pos, ss_head;
};
void paged_prefill_attention(const PrefillAttnArgs& a, hipStream_t s);

// ---- batched token sampling (sampling.hip) ----------------------------------
// out[b] = one token of row b of logits [b, v] (bf16 | fp32, unit inner
// stride, row_stride in elements, rows need no alignment), 1 <= v < 2^23.
// One launch, one block per row; no sort, no workspace, no host read.  The
// result is exact: it does not depend on thread count or summation order.
//   Order.   Tokens are ordered by (logit descending, index ascending); NaN
//            orders lowest, -0 == +0.
//   Greedy.  temperature <= 0 (or NaN), top_k == 1 or top_p <= 0: the first
//            token in the order.  No random number is used.
//   Weights. w_i = 2^40 for every element equal to the row maximum, else
//            rint(2^40 * exp2((x_i - max) * (log2(e) / T))) in fp32 as u64
//            (0 for a NaN); Z = sum w_i < 2^63.  All later sums are integer.
//            A token with w_i = 0, probability under 2^-41 of the maximum's,
//            cannot be drawn.
//   Kept.    Token kept iff the weight strictly before it in the order is
//            < ceil(fp64(top_p) * fp64(Z)) (top_p >= 1 keeps all) and, with
//            top_k > 0, its rank is < top_k.  Equal logits are kept lowest
//            index first.  The first token is always kept.
//   Draw.    r = rand_bits[b] as u64 when rand_bits != null, else
//            (x[0] << 32 | x[1]) of x = philox10(seed[b], offset[b]);
//            t = mulhi64(r, Z_S), Z_S the kept weight; the result is the
//            lowest kept index whose inclusive prefix sum of kept weights in
//            INDEX order exceeds t.
// Rows whose keys fit 128 KB (v <= 65536 bf16, 32768 fp32) stay in LDS after
// one global read; longer rows re-read global memory on every pass.
struct SampleArgs {
  const void* logits;
  const float *temperature, *top_p;
  const int* top_k;                  // <= 0: off
  const int64_t *seed, *offset;
  const int64_t* rand_bits;          // null: Philox
  int64_t* out;
  int b, v;
  long long row_stride;
  int dtype;
};
void sample_tokens(const SampleArgs& a, hipStream_t s);

// ---- dense MFMA GEMM (gemm.hip bf16, gemm_fp8.hip e4m3) --------------------
// C[z] = op(A[z]) x op(B[z]) for z = 0 .. batch-1, fp32 accumulate, bf16 C.
//   layout  kGemmNT: A[m][k], Bt[n][k]   kGemmNN: A[m][k], B[k][n]
//           kGemmTN: At[k][m], B[k][n] (wgrad).  fp8 is NT only.
//   bf16 epilogue: none | + bias[n] | gelu(x + bias), pre-activation written
//     to aux | x * gelu'(aux).  accumulate: C += result, epilogue none.
//   fp8: C = scale_ab * (A x Bt^T) (+ bias[n] when bias != null); operands
//     are OCP e4m3 bytes; epilogue / accumulate / aux are not read.
// Contract (checked by the binding before any launch, docs/KERNELS.md):
//   * a, b, bias, aux, c on one GPU; bias, aux, c bf16.
//   * all rows have unit inner stride; lda / ldb / ldc are row strides and
//     *_bs batch strides, in elements.
//   * a and b are staged by 16-byte accesses (DMA and guarded vector loads)
//     through lda / ldb / a_bs / b_bs: each is a multiple of 16 bytes (8 bf16,
//     16 fp8) and the a / b base pointers are 16-byte aligned.  c, aux and
//     bias are accessed element by element and need neither.
//   * k >= 64 (bf16) or 128 (fp8); 1 <= m, n, k < 2^31; 1 <= batch <= 65535.
//   * bias non-null exactly when the epilogue reads it: n elements, advanced
//     by bias_bs per batch (fp8; the bf16 kernel shares one bias).
//   * aux [m][n] with row stride ldc for the two GELU epilogues.
enum GemmLayout : int { kGemmNT = 0, kGemmNN = 1, kGemmTN = 2 };
enum GemmEpilogue : int {
  kGemmEpiNone = 0, kGemmEpiBias = 1, kGemmEpiBiasGelu = 2, kGemmEpiDGelu = 3
};
struct GemmArgs {
  const void *a, *b;
  void* c;
  const void* bias;
  void* aux;
  int64_t m, n, k;
  int64_t lda, ldb, ldc;
  int64_t batch;                       // grid.z; 1 = plain GEMM
  int64_t a_bs, b_bs, c_bs, bias_bs;
  int layout, epilogue;
  bool accumulate;
  float scale_ab;                      // fp8 only
};
void gemm_bf16(const GemmArgs& g, hipStream_t s);
void gemm_fp8(const GemmArgs& g, hipStream_t s);
// bf16 -> e4m3 cast with uniform scale (fused, no fp32 round-trip).  x is
// contiguous bf16, numel a multiple of 8.  v = fp32(x) * scale is rounded to
// nearest even, subnormals (down to 2^-9) and the sign of zero included.
// Out of range, as measured on gfx950 (tests/test_quant_fp8_gpu.py): the
// conversion rounds first, so 448 < |v| <= 464 gives +-448 (0x7E / 0xFE); from
// |v| = 480 on, +-Inf included, it gives the NaN byte with v's sign (0x7F /
// 0xFF), it does NOT saturate; NaN gives a NaN byte.  With scale =
// fp32(448) / fp32(amax) the largest element is at most one fp32 ulp above
// 448 and comes out as +-448 for every bf16 amax, so the per-tensor recipe
// (incubate/fp8.py) needs no clamp; a caller with another scale must clamp.
void quant_fp8(const void* x, void* out, float scale, int64_t numel,
               hipStream_t s);

// ---- MXFP4 GEMM (gemm_mx.hip) -----------------------------------------------
// OCP microscaling fp4.  codes uint8 [R, K/2]: byte i of a row holds element
// 2i in the low nibble and 2i+1 in the high one (e2m1: sign, 2-bit exponent,
// 1-bit mantissa; magnitudes 0 .5 1 1.5 2 3 4 6).  scales uint8 [R, K/32]
// e8m0, one per 32 elements along K: 2^(byte - 127).
// gemm_mxfp4: C[m][n] = sum_k A[m][k] * Bt[n][k] (+ bias[n]), fp32
//   accumulate, bf16 C.  Reads of GemmArgs: a, b (codes), c, bias, m, n, k
//   (ELEMENTS), lda / ldb (BYTES of codes per row), ldc; batch must be 1;
//   scale_ab, epilogue, layout, accumulate and aux are not read.  sa [m][k/32]
//   and sb [n][k/32] with row strides ldsa / ldsb in bytes.
// Contract (checked by the binding before any launch or allocation):
//   * everything on one GPU; codes and scales uint8 with unit inner stride;
//   * code rows (lda, ldb) and the a / b base pointers 16-byte aligned; ldsa,
//     ldsb and the sa / sb base pointers even (the kernel loads scale pairs);
//   * k % 128 == 0, 128 <= k < 2^31, 1 <= m, n < 2^31; bias bf16 [n] or null.
//   * k % 256 != 0 runs the guarded kernel over the whole grid (slow path).
// mx_quant_fp4: x bf16 [rows, k] with row stride ld elements (ld % 8 == 0,
//   base 16-byte aligned, k % 32 == 0, finite values) -> contiguous codes
//   [rows, k/2] and scales [rows, k/32].  Per block: e = floor(log2 amax) - 2
//   from the exponent bits of amax, clamped to [-127, 127]; scale byte e +
//   127; amax == 0 gives byte 127 and zero codes; each element is x * 2^-e
//   rounded to the nearest grid value, ties to the even code, saturating at 6.
//   One read pass, no atomics, no workspace, no host read.
void gemm_mxfp4(const GemmArgs& g, const uint8_t* sa, const uint8_t* sb,
                int64_t ldsa, int64_t ldsb, hipStream_t s);
void mx_quant_fp4(const void* x, void* codes, void* scales, int64_t rows,
                  int64_t k, int64_t ld, hipStream_t s);
// one-wave layout probe of the e2m1 scaled MFMA: a, bt [16][64] codes, sa, sb
// [16][4] scale bytes, c [16][16] fp32, opsel 0..3 the scale byte position
void mfma_probe_fp4mx(const void* a, const void* bt, const void* sa,
                      const void* sb, float* c, int opsel, hipStream_t s);

// MFMA W-streaming decode GEMMs (decode_gemm.hip) for three weight formats.  1 <= M <= 32, N % 256 == 0, K % 64 == 0, K <= 2^24;
// x bf16 [M, K] contiguous; x and weight base pointers 16-byte aligned.
// ksplit 0 = heuristic.  `workspace` holds [decode_split_plan(k, n,
// ksplit).splits, padded_m, N] fp32 with padded_m = 16 (M <= 16) or 32.
struct DecodeSplitPlan { int kchunk, splits; };
DecodeSplitPlan decode_split_plan(int64_t k, int64_t n, int64_t ksplit);
// w bf16 [K, N] with row stride ldw, ldw % 8 == 0
void decode_gemm_mfma(const void* x, const void* w, const void* bias, void* y,
                      float* workspace, int64_t m, int64_t n, int64_t k,
                      int64_t ldw, int64_t ksplit, hipStream_t s);
// qw int8 [K, N] contiguous, scale fp32 [N]; w ~ code * scale / 127
void decode_gemm_int8(const void* x, const void* qw, const float* scale,
                      const void* bias, void* y, float* workspace, int64_t m,
                      int64_t n, int64_t k, int64_t ksplit, hipStream_t s);
// qw int8 [K/2, N] contiguous: byte (kp, n) = code[2kp, n] in the low
// nibble, code[2kp+1, n] in the high one, codes -7..7; scale fp32 [N]
// (group_size -1) or [K/gs, N] (gs 64 | 128), K % gs == 0;
// w ~ code * scale / 7
void decode_gemm_int4(const void* x, const void* qw, const float* scale,
                      const void* bias, void* y, float* workspace, int64_t m,
                      int64_t n, int64_t k, int64_t group_size, int64_t ksplit,
                      hipStream_t s);
// packed [K/2, N] + scales -> bf16 | fp32 [K, N]; N % 8 == 0.  Each element
// is float(code) * (scale * fp32(1/7)).
void dequant_int4(const void* qw, const float* scale, void* out, int64_t k,
                  int64_t n, int64_t group_size, int dtype, hipStream_t s);

// ---- MXFP4 weight-only decode streamer (decode_gemm_mx.hip) -----------------
// decode_gemm_mxfp4: y[M,N] = x[M,K] . dequant(qw, scales)^T (+ bias[N]); x, y,
//   bias bf16, fp32 accumulate; only the weight is fp4 (x is not quantized).
//   qw / scales in the MXFP4 GEMM format above with R = N: codes [N, K/2],
//   e8m0 scales [N, K/32].  `workspace` holds [decode_mx_split_plan(k, n,
//   ksplit).splits, padded_m, N] fp32 with padded_m = 16 (M <= 16) or 32; rows
//   < M of it are written in full before the reduce kernel reads them.
//   ksplit 0 = heuristic; kchunk is a multiple of 128.  No atomics, no host
//   read.
// Contract (checked by the binding before any launch or allocation):
//   * everything on one GPU;
//   * x bf16 [M, K] contiguous and 16-byte aligned, 1 <= M <= 32;
//   * qw uint8 [N, K/2] contiguous and 16-byte aligned;
//   * scales uint8, exactly [N, K/32], contiguous and 4-byte aligned;
//   * K % 128 == 0, 128 <= K <= 2^24; N % 64 == 0, N >= 64;
//   * bias bf16 contiguous [N] or null; ksplit >= 0.
//   * scale bytes in [8, 247] (what mx_quant_fp4 writes for bf16-normal
//     weights; not scanned): inside it every weight is converted exactly,
//     outside it the result is unspecified but memory-safe.
// mx_dequant_fp4: codes [rows, k/2] + scales [rows, k/32], both contiguous,
//   codes 16-byte aligned, k % 32 == 0 -> out bf16 [rows, k] contiguous;
//   exact for the same scale range.
DecodeSplitPlan decode_mx_split_plan(int64_t k, int64_t n, int64_t ksplit);
void decode_gemm_mxfp4(const void* x, const void* qw, const void* scales,
                       const void* bias, void* y, float* workspace, int64_t m,
                       int64_t n, int64_t k, int64_t ksplit, hipStream_t s);
void mx_dequant_fp4(const void* codes, const void* scales, void* out,
                    int64_t rows, int64_t k, hipStream_t s);

// ---- MoE routing (assign_pos/number_count/gate parity) --------------------
void moe_gate_topk(const float* logits, float* topv, int* topi, float* me,
                   float* ce, int64_t t, int64_t e, int64_t k, hipStream_t s);
void moe_assign_slots(const int* topi, int* slot_of, int* counts, int64_t t,
                      int64_t e, int64_t k, int64_t cap, hipStream_t s);

// ---- MoE dispatch / combine over collision-free slot maps -------------------
// moe_route (moe.hip): topi int32 [T, K] -> slot_of [T, K], src_of [E * cap],
// counts [E], all int32 and all written in full by the kernel.  In GShard
// order, pos(t, kk) = #{(t', kk') : topi[t', kk'] == topi[t, kk] and
// (kk', t') < (kk, t)}; slot_of[t, kk] = e * cap + pos if pos < cap else -1;
// src_of[e * cap + pos] = t * K + kk, -1 on the empty tail; counts[e] counts
// dropped entries too.  An id outside [0, E) gets slot -1 and is not counted.
// block_waves: waves per expert block, 1 | 4 | 16, 0 = by problem size.
void moe_route(const int* topi, int* slot_of, int* src_of, int* counts,
               int64_t t, int64_t e, int64_t k, int64_t cap, int block_waves,
               hipStream_t s);
// Row movers (moe_permute.hip).  slots = E * cap.
//   moe_dispatch:    out[s] = x[src_of[s] / K], zeros for an empty slot; x
//                    [T, h], out [slots, h]; a bit copy.
//   moe_combine:     out[t] = sum_kk w[t, kk] * x[slot_of[t, kk]] over kept kk,
//                    fp32 accumulation, one rounding; x [slots, h], out [T, h];
//                    w null = weight 1 (the backward of dispatch).
//   moe_combine_bwd: out[s] = w[src] * dout[t] and dw[src] = <x[s], dout[t]>
//                    in fp32 for src = src_of[s] kept, t = src / K; else
//                    out[s] = 0.  x = y [slots, h], dout [T, h], out = dy
//                    [slots, h]; dw [T, K] comes in zeroed.
// Contract (checked by the binding before any launch or allocation,
// docs/KERNELS.md "MoE dispatch / combine"):
//   * all tensors on one GPU;
//   * rows (x, dout, out) bf16 or fp32, one dtype per call, contiguous
//     [., h], 16-byte aligned, h % 8 == 0;
//   * maps int32 and contiguous, slot_of [T, K], src_of [slots];
//   * w and dw fp32 contiguous [T, K];
//   * 1 <= K <= 8, E >= 1, cap >= 1, T * K < 2^31, E * cap < 2^31;
//   * T == 0 returns empty or zero outputs without a launch.
// A src_of entry outside [0, T * K) counts as empty and a slot_of entry
// outside [0, slots) as dropped; neither is used as an index.
struct MoePermuteArgs {
  const void* x;
  const void* dout;
  const float* w;
  const int *slot_of, *src_of;
  void* out;
  float* dw;
  int t, k, slots, h, dtype;
};
void moe_dispatch(const MoePermuteArgs& a, hipStream_t s);
void moe_combine(const MoePermuteArgs& a, hipStream_t s);
void moe_combine_bwd(const MoePermuteArgs& a, hipStream_t s);

// ---- dropless MoE: compact route + ragged grouped GEMM ------------------------
// moe_route_ragged (moe.hip): topi int32 [T, K] -> slot_of [T, K], src_of
// [T * K], offsets [E + 1], all int32 and all written in full by the kernel.
// pos(t, kk) as in moe_route; offsets[e] = number of valid ids below e (the
// exclusive prefix sum of the per-expert counts), offsets[E] = number of valid
// entries; slot_of[t, kk] = offsets[e] + pos, nothing is dropped;
// src_of[slot] = t * K + kk; an id outside [0, E) gets slot -1 and the rows
// [offsets[E], T * K) of src_of are -1.  No atomics, no host read.
void moe_route_ragged(const int* topi, int* slot_of, int* src_of, int* offsets,
                      int64_t t, int64_t e, int64_t k, hipStream_t s);

// grouped_gemm_bf16 (grouped_gemm.hip): bf16 in, fp32 accumulate, bf16 out over
// `rows` = R rows sorted by group; group e owns rows [offsets[e], offsets[e+1]),
// read on the device.
//   kGroupedNN  C[r, :] = A[r, :] . B[g(r)] (+ bias[g(r), :])
//               A [R, k], B [E, k, n] (b_gs, ldb), bias [E, n] (ldbias), C [R, n]
//   kGroupedNT  C[r, :] = A[r, :] . B[g(r)]^T     A [R, k], B [E, n, k], C [R, n]
//   kGroupedTN  C[e] = sum_{r in e} A[r, :]^T (x) B[r, :]
//               A [R, m], B [R, n], C [E, m, n] (c_gs, ldc); an empty group
//               gives zeros; one block sums a group in row order, no atomics
// NN / NT take the tile map that grouped_gemm_plan wrote from the same
// offsets: grouped_gemm_map_tiles(R, E) int32 pairs (group, first row), one
// launch, every element written; one map serves every NN / NT call of a route.
// Rows [offsets[E], R) of an NN / NT output are written as zeros; every output
// element is written, outputs need no initialisation.
// Contract (checked by the binding before any launch or allocation):
//   * everything on one GPU; a, b, c, bias bf16 with unit inner stride,
//     16-byte aligned bases, row strides and group strides;
//   * k, n, m multiples of 64 and >= 64; 1 <= E <= 1024; R < 2^31;
//   * offsets int32 contiguous [E + 1]; tile_map int32 contiguous
//     [grouped_gemm_map_tiles(R, E), 2];
//   * R == 0 launches nothing.
// Offsets are not trusted: group e covers [clamp(o_e), clamp(max(o_e+1, o_e)))
// with clamp to [0, R]; malformed offsets or a foreign map give an
// unspecified but memory-safe result.
constexpr int kGroupedGemmBM = 128;
enum GroupedForm : int { kGroupedNN = 0, kGroupedNT = 1, kGroupedTN = 2 };
struct GroupedGemmArgs {
  const void *a, *b;
  void* c;
  const void* bias;                    // NN only, may be null
  const int *offsets, *tile_map;       // tile_map: NN / NT
  int64_t rows, groups, m, n, k;
  int64_t lda, ldb, ldc, ldbias;
  int64_t b_gs, c_gs;                  // group strides of B (NN / NT), C (TN)
  int form;
};
int64_t grouped_gemm_map_tiles(int64_t rows, int64_t groups);
void grouped_gemm_plan(const int* offsets, int* tile_map, int64_t rows,
                       int64_t groups, hipStream_t s);
void grouped_gemm_bf16(const GroupedGemmArgs& a, hipStream_t s);

}  // namespace pa
