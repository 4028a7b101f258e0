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
};
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
// bf16 -> e4m3 cast with uniform scale (fused, no fp32 round-trip)
void quant_fp8(const void* x, void* out, float scale, int64_t numel,
               hipStream_t s);

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

// ---- MoE routing (assign_pos/number_count/gate parity) --------------------
void moe_gate_topk(const float* logits, float* topv, int* topi, float* me,
                   float* ce, int64_t t, int64_t e, int64_t k, hipStream_t s);
void moe_assign_slots(const int* topi, int* slot_of, int* counts, int64_t t,
                      int64_t e, int64_t k, int64_t cap, hipStream_t s);

}  // namespace pa
