// Host-side launch API of the gfx950 kernels.  Plain pointers + hipStream_t only,
// so the kernel translation units never include torch headers; bindings.cpp is
// the only file that knows about at::Tensor.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gemm_plan.h"

struct AttnFwdArgs {
  const uint16_t *q, *k, *v;
  uint16_t* o;
  float* lse;  // [B, H, T] natural-log LSE, may be null
  int B, H, Hkv, T, S, D;
  int64_t q_sb, q_st, q_sh, k_sb, k_st, k_sh, v_sb, v_st, v_sh, o_sb, o_st, o_sh;
  float scale, scale_log2;
  int causal;
  unsigned long long* stamps;  // diagnostic builds only (PLLM_FWD_STAMPS): per-wave phase cycles
  // optional per-row key bounds (document / window masks; causal, S == T): query i sees keys
  // kv_start[b, i] <= j <= i.  int32 [B, T], non-decreasing along T, 0 <= kv_start[i] <= i.  Null: plain causal
  const int* kv_start;
  // optional attention sinks: bf16 [H], one logit per query head added to every row's softmax denominator
  // (no value row, not scaled).  Null: plain softmax
  const uint16_t* sinks;
};

// q [B, H, D] (one query per sequence), k/v rows of a [B, S_max, Hkv, D]-strided cache
struct DecodeArgs {
  const uint16_t *q, *k, *v;
  uint16_t* o;
  float *part_o, *part_lse;  // [B, H, splits, D] / [B, H, splits] when splits > 1
  const int* seqlen;         // optional device key count (graph capture); else S
  int seqlen_per_row;        // seqlen holds B counts (one per sequence) instead of one
  int B, H, Hkv, S, D, splits;
  int64_t q_sb, q_sh, k_sb, k_st, k_sh, v_sb, v_st, v_sh, o_sb, o_sh;
  float scale_log2;
  int window;                // sliding window: only the last `window` keys of the count are read (0 = all)
  const uint16_t* sinks;     // optional attention sinks, bf16 [H] (see AttnFwdArgs), folded in once at the last merge
};

struct AttnBwdArgs {
  const uint16_t *q, *k, *v, *o, *dO;
  const float* lse;
  // optional RoPE (rotate-half) fp32 tables [>= S, D/2]: q / k arrive rotated (query row t at position
  // t + S - T, key row j at position j) and dq / dk leave un-rotated
  const float *rope_cos, *rope_sin;
  float* delta;   // [B, H, T] scratch
  uint16_t* dq_acc;  // [nkb_pass][B, T, H, D] bf16 per-key-block dQ partial slabs of one pass
  float* dq_sum;  // [B, T, H, D] fp32 running dQ sum across passes (null when one pass)
  int kb0, nkb_pass;  // first key block of the pass / key blocks per pass (set by the host)
  int64_t slab;       // elements per dQ slab (>= B * ceil32(T) * H * D)
  int nqt;            // ceil(T / 32): query tiles per head in the fragment-order slab
  uint16_t *dq, *dk, *dv;
  int B, H, Hkv, T, S, D;
  int64_t q_sb, q_st, q_sh, k_sb, k_st, k_sh, v_sb, v_st, v_sh, o_sb, o_st, o_sh, do_sb, do_st, do_sh;
  int64_t dq_sb, dq_st, dq_sh, dk_sb, dk_st, dk_sh, dv_sb, dv_st, dv_sh;
  float scale, scale_log2;
  int causal;
  unsigned long long* stamps;  // diagnostic builds only (PLLM_BWD_STAMPS): per-wave phase cycles
  int delta_ready;             // 1: delta already holds rowsum(dO * O) (gemm_tn epilogue 6): no pre-pass
  // optional per-row key bounds (see AttnFwdArgs; both or neither): q_last[b, j] int32 [B, S] is the last
  // query that sees key j, so visibility is kv_start[i] <= j <= i  <=>  j <= i <= q_last[j]
  const int *kv_start, *q_last;
};

namespace pllm {

// norm.hip
void norm_fwd(const void* x, const void* res, const void* w, const void* b, void* y, void* s, float* mean,
              float* rstd, int N, int C, float eps, bool rms, hipStream_t st);
int norm_bwd_grid(int N, int C);
// xb_part/xb: optional column sums of dx (bias grad of the layer that produced x)
// Gradient outputs (dw, db, xb, bias grads, wgrad, embedding grads) are bf16 or fp32 (grad_f32 /
// out_f32: the optimizer's flat-gradient dtype); activations and their gradients are bf16.
void norm_bwd(const void* dy, const void* s, const void* w, const float* mean, const float* rstd, const void* ds,
              void* dx, float* dw_part, float* db_part, void* dw, void* db, bool grad_f32, int N, int C, bool rms,
              bool accumulate, float* xb_part, void* xb, bool xb_accumulate, hipStream_t st);
// fp32 [G, C] slab -> [C] column sums (bf16 or fp32 out; optionally added into out)
void col_reduce(const float* part, int G, int C, void* out, bool out_f32, bool accumulate, hipStream_t st);
// bias gradient = column sums of a bf16 [N, C] matrix; part: fp32 [colsum_groups(N), C] workspace
int colsum_groups(int N);
void bias_grad(const void* x, int N, int C, float* part, void* out, bool out_f32, bool accumulate, hipStream_t st);

// elementwise.hip (op: 0 relu, 1 gelu-tanh)
void act_fwd(int op, const void* x, void* y, size_t n, hipStream_t st);
void act_bwd(int op, const void* dy, const void* xin, void* dx, size_t n, hipStream_t st);
// activation backward + fused bias gradient (column sums of dx) of the producing linear layer
void act_bwd_bias(int op, const void* dy, const void* xin, void* dx, int N, int C, float* part, void* bias_grad,
                  bool grad_f32, bool accumulate, hipStream_t st);
void swiglu_fwd(const void* gu, void* y, size_t rows, int F, hipStream_t st);
void swiglu_bwd(const void* dy, const void* gu, void* dgu, size_t rows, int F, hipStream_t st);
void rope(const void* in, void* out, const float* cosb, const float* sinb, size_t rows, int T, int n_heads_total,
          int n_rot, int D, int pos_offset, bool inverse, hipStream_t st, int out_heads = 0);
void scale_inplace(void* x, bool f32, const float* s, size_t n, hipStream_t st);  // x *= s[0] (no-op when 1)
// ring-attention LSE merge; st: element strides of o_acc (b, t, h), lse_acc (b, h, t), o (b, t, h), lse (b, h, t)
// zero n byte ranges of buf (desc int64 [n][3] on the device = start, end, bytes of the ranges before; 16-B
// aligned); total_bytes: all ranges together
void zero_ranges(void* buf, const int64_t* desc, int n, int64_t total_bytes, hipStream_t st);
void lse_merge(float* o_acc, float* lse_acc, const void* o, const float* lse, const int64_t* st, int B, int T, int H,
               int D, hipStream_t stream);

// qk_norm.hip: per-head RMSNorm of the q / k heads of packed qkv rows [rows, (H + 2 Hkv) D], fused into the
// attention's RoPE pre-pass.  Forward: qk [rows, (H + Hkv) D] = rotate(x rstd gamma) (no rotation when cosb is
// null), rstd fp32 [rows, H + Hkv].  Backward: in place on the q / k columns of dqkv (dy -> dx), the gain
// gradients through fp32 partials part [2][qk_norm_bwd_grid()][D] and col_reduce (deterministic).
void qk_norm_rope(const void* qkv, const void* wq, const void* wk, void* qk, float* rstd, const float* cosb,
                  const float* sinb, size_t rows, int T, int H, int Hkv, int D, int pos_offset, float eps,
                  hipStream_t st);
int qk_norm_bwd_grid(size_t rows, int H, int Hkv, int D);
void qk_norm_bwd(void* dqkv, const void* qkv, const float* rstd, const void* wq, const void* wk, size_t rows, int H,
                 int Hkv, int D, float* part, void* dwq, void* dwk, bool grad_f32, bool accumulate, hipStream_t st);

// cross_entropy.hip
void cross_entropy(const void* logits, int64_t ld, const int64_t* targets, int N, int V, int ignore_index,
                   float* loss, void* dlogits, const float* inv_n, hipStream_t st);
// the same with an auxiliary z-loss (loss += z_loss * lse^2) and final-logit soft-capping (softcap * tanh(x / softcap),
// 0: off); lse (optional): fp32 [N], the rows' log-sum-exp (0 on ignored rows)
void cross_entropy_aux(const void* logits, int64_t ld, const int64_t* targets, int N, int V, int ignore_index,
                       float* loss, void* dlogits, const float* inv_n, float z_loss, float softcap, float* lse,
                       hipStream_t st);
int cross_entropy_max_vocab();

// adamw.hip
void adamw_flat(void* param_bf16, float* master, float* m, float* v, const void* grad, bool grad_f32, size_t n,
                float lr, float b1, float b2, float eps, float wd, int step, float grad_scale,
                const float* scale_ptr, const uint8_t* wd_blocks, const float* hyper, hipStream_t st);
int sumsq_blocks(size_t n);
void sumsq(const void* x, bool f32, size_t n, float* part, hipStream_t st);
// out[0] = sqrt(sum(part[0..G))) * grad_scale (the gradient norm), out[1] = min(max_norm / (out[0] + 1e-6), 1)
void clip_coef(const float* part, int G, float grad_scale, float max_norm, float* out, hipStream_t st);

// embedding.hip
void embedding_fwd(const int64_t* idx, const void* wte, const void* wpe, void* out, int64_t N, int T, int C,
                   int pos_offset, int64_t V, hipStream_t st);
int64_t embedding_bwd_chunks(int64_t N);  // fp32 workspace: 2 * chunks * C floats
void embedding_bwd(const void* dx, const int32_t* sorted, const int32_t* perm, void* dwte, void* dwpe, bool grad_f32,
                   float* part, int64_t N, int Bn, int T, int C, int64_t V, hipStream_t st);

// gemm.hip / gemm_pp.hip: C[M,N] = epi(A[M,K] B[N,K]^T), epi 0..7 as listed at the top of gemm.hip;
// 3 / 4 write column sums of C to colpart [GemmPlan::colsum_groups][N] (fp32)
struct GemmArgs {
  const uint16_t* A;
  const uint16_t* B;
  uint16_t* C;
  const uint16_t* bias;
  uint16_t* aux;
  float* colpart;
  int64_t lda, ldb, ldc, ldaux;
  int M, N, K;
  int group_m;  // set by gemm_tn
  float* delta;  // epilogue 6: [M / T, N / 64, T] row sums of C * aux per 64-column head
  int T;         // epilogue 6: rows per sequence
};
// The dispatch settings (gemm_plan.h) and the device's CU count: what gemm_plan / wgrad_plan take.
// gemm_settings() re-reads the PLLM_AB key wgrad_hy_cost on every call.
const GemmSettings& gemm_settings();
int gemm_cus();
// phased: 0 single-phase, 2 asym DMA, 4 ping-pong kernel (gemm_pp.hip); reserve_cus >= 0: CUs left
// free by the persistent grids (collectives in flight), -1 keeps the current setting
void gemm_set_config(int mfma, int group_m, int phased, int reserve_cus = -1, int persistent = -1);
// 0: default dispatch; 16 / 32: gemm_wgrad.hip's kernel with that MFMA shape; any other value (100): that
// kernel with the MFMA shape chosen per problem
void wgrad_set_mfma(int mf);
void wgrad_set_hy(int on);  // A/B: hybrid weight gradients where they apply
// p = gemm_plan(gemm_settings(), gemm_cus(), a.M, a.N, a.K, epi, a.T)
void gemm_tn(const GemmArgs& a, const GemmPlan& p, int epi, hipStream_t st);
void gemm_tn_pp(const GemmArgs& a, const GemmPlan& p, int epi, hipStream_t st);  // gemm_pp.hip
// gemm_wgrad.hip: dW[P,Q] (+)= dY[M,P]^T X[M,Q] under p = wgrad_plan(gemm_settings(), gemm_cus(), M, P, Q,
// out_f32, bpart && bout); part: p.ws_floats fp32 workspace.  bpart / bout (optional): also the bias gradient
// db[P] (+)= column sums of dY, through an fp32 [p.bias_rows][P] workspace; returns p.fused_bias, whether
// it was computed
bool wgrad(const WgradPlan& p, const void* dy, int64_t lda, const void* x, int64_t ldb, int M, int P, int Q,
           float* part, void* out, bool out_f32, bool accumulate, hipStream_t st, float* bpart = nullptr,
           void* bout = nullptr, bool bout_f32 = false);
// wgrad_pp.hip: the ping-pong weight-gradient kernel (fp32 targets; arms 2 and 3 of wgrad()) and, on arm 3
// (no bias, more tiles than workgroups: whole tiles for the grid's whole rounds, slices for the last one),
// its ordered fix-up
void wgrad_pp(const WgradPlan& p, const void* dy, int64_t lda, const void* x, int64_t ldb, int M, int P, int Q,
              float* part, float* out, bool accumulate, float* bpart, hipStream_t st);
// wgrad_pp.hip, grouped arm: whole tiles [first, last) of the global tile list of up to kWgradGroupMax problems
// (pre[i]: index of problem i's first tile, pre[np] the total; a problem's tiles row band by row band), each tile
// stored into / added to its problem's fp32 gradient by the workgroup that ran all its K-tiles.  bias_out (or
// null): the problem's fp32 bias gradient, which the first Q tile of every row band adds its column sums to.
// The argument travels by value: no table in device memory, nothing for a graph capture to re-read.
struct WgradGroupProblem {
  const void* A;  // dY [M, P], row stride lda
  const void* B;  // X [M, Q], row stride ldb
  int64_t lda, ldb;
  float* out;       // [P, Q]
  float* bias_out;  // [P] or null
  int M, P, Q;
  int accumulate;   // out += tile (else out = tile)
};
struct WgradGroup {
  WgradGroupProblem p[kWgradGroupMax];
  int pre[kWgradGroupMax + 1];
  int np, first, last;
};
void wgrad_pp_group(const WgradGroup& g, int grid, hipStream_t st);

// transpose.hip: desc int64 [n][6] = (src, dst, rows, cols, first tile, tiles per row band)
int transpose_tiles(int R, int C);
void transpose_batch(const int64_t* desc, int n, int total_tiles, hipStream_t st);

// sampling.hip: Gumbel-max draw of one token per row of logits [B, V] (temperature <= 0: argmax)
void sample_tokens(const void* logits, bool bf16_in, int64_t ld, int B, int V, float temperature, uint64_t seed,
                   int64_t* out, hipStream_t st);

// sampling_rows.hip: per-row temperature / top-k / top-p / min-p Gumbel-max draw, every parameter a
// device array of B entries; uniforms keyed by (seed[row], step[row], column) only
void sample_rows(const void* logits, bool bf16_in, int64_t ld, int B, int V, const float* temperature,
                 const int* top_k, const float* top_p, const float* min_p, const int64_t* seed, const int64_t* step,
                 int64_t* tokens, int* kept, float* min_kept, hipStream_t st);

// gemv.hip: y[M, N] = act(in[M, K] W[N, K]^T + bias) for M <= gemv_max_rows() (decode projections),
// in = x, or norm(x + res) with the residual stream x + res written to s_out when gamma is set.
// gemv_fp8: W is given as OCP e4m3fn codes (one byte each, ldw in bytes) with one fp32 scale per row:
// y = act((in . codes^T) * wscale + bias)
struct GemvArgs {
  const uint16_t* x;
  int64_t ldx;
  const uint16_t* res;    // nullable (NORM only)
  int64_t ldr;
  const uint16_t* gamma;  // nullable: no norm prologue
  const uint16_t* beta;   // nullable: RMSNorm / no shift
  uint16_t* s_out;        // nullable: x + res
  int64_t lds;
  float eps;
  int rms;
  const void* w;          // bf16 (gemv) or e4m3fn codes (gemv_fp8); ldw in elements
  int64_t ldw;
  const uint16_t* bias;   // nullable
  uint16_t* y;
  int64_t ldy;
  int N, K, Mr;
  int act;  // 0 none, 1 GELU (tanh), 2 ReLU
  // decode KV-cache append (nullable kc): output columns [q_cols, q_cols + kv_cols) of row m
  // also go to kc[m, *pos, :], the next kv_cols to vc[m, *pos, :] (caches [B, S_max, kv_cols])
  uint16_t* kc;
  uint16_t* vc;
  const int64_t* pos;
  int pos_per_row;  // pos holds one position per row (continuous batching) instead of one
  int64_t kv_ldb;
  int q_cols, kv_cols, kv_smax;  // positions outside [0, kv_smax) are dropped, never written
  const float* wscale;  // nullable: gemv_fp8 only, one scale per row of w [N] (last: the bf16 kernels' argument layout stays)
};
int gemv_max_rows();
void gemv(const GemvArgs& a, hipStream_t st);
void gemv_fp8(const GemvArgs& a, hipStream_t st);

// quant_fp8.hip: per-row weight quantiser of the FP8 decode path.  scale[n] = max_k |w[n, k]| / 448 (1 for an
// all-zero row), q[n, k] = the e4m3fn code nearest to w[n, k] / scale[n] (ties to even)
void quantize_rows_fp8(const uint16_t* w, int64_t ldw, uint8_t* q, float* scale, int N, int K, hipStream_t st);

// attention.hip
bool attn_supported_head_dim(int D);
constexpr int kAttnBwdKeyBlock = 256;  // keys per backward workgroup = dq_acc slab count divisor
// attn_bwd_ks.hip: one pass of the key-stationary main kernel, D = 128 (AttnBwdArgs as attn_bwd)
void attn_bwd_ks_launch(const AttnBwdArgs& a, hipStream_t st);
// attn_decode.hip: split-KV single-query attention over a KV cache
bool attn_decode_supported(int D, int group);
int attn_decode_splits(int B, int Hkv, int S_max);
void attn_decode(const DecodeArgs& a, hipStream_t st);
void attn_fwd(const AttnFwdArgs& a, hipStream_t st);
void attn_bwd(const AttnBwdArgs& a, hipStream_t st);
// attn_sink.hip: sink gradient ds[h] = -sum_{b,t} exp(s[h] - lse[b,h,t]) delta[b,h,t] (lse, delta fp32 [B, H, T],
// sinks bf16 [H]) through fp32 partials part [attn_sink_bwd_grid()][H] and col_reduce (deterministic)
int attn_sink_bwd_grid(int B, int T);
void attn_sink_bwd(const float* lse, const float* delta, const void* sinks, int B, int H, int T, float* part,
                   void* out, bool out_f32, bool accumulate, hipStream_t st);

}  // namespace pllm
