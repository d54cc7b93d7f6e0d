// The host boundary of the kernel library: the one declaration of every extern "C" rn_* launcher.
//
// Included by the unit that defines a launcher (csrc/kernels/*.hip) and by every unit that calls one
// (csrc/bindings/*.cpp, csrc/comm/*.cpp, other kernel units and headers), so the compiler sees the
// prototype and the definition together: a parameter list that changes on one side only is a
// "conflicting types" build error instead of shifted arguments at run time.  Plain C++ — no torch and
// no device headers.
//
// Conventions: pointers are device pointers unless noted; bf16 tensors travel as void*; an optional
// pointer may be null; element counts, sizes and strides are in elements unless a comment says bytes;
// launchers that return a status return 0 on success and a non-zero code for a shape / argument they
// do not take (nothing launched); `st` is the stream every launch goes to.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

extern "C" {

// ------------------------------------------------------------------ elementwise.hip
void rn_cast_f32_bf16(const float* in, void* out, long n, hipStream_t st);
// kind: the ACT_* code of common.h
void rn_act_fwd(const void* x, void* y, long n, int kind, hipStream_t st);
void rn_act_bwd(const void* dy, const void* x, void* dx, long n, int kind, hipStream_t st);
// seed_ptr (optional): 1 device uint64 read instead of `seed`, so a captured graph replays with a fresh draw
void rn_dropout(const void* x, void* y, long n, float p, uint64_t seed, const uint64_t* seed_ptr, hipStream_t st);
// Device RNG stream for dropout seeds: out[0] = splitmix64(state[0]); state[0] += γ (both 1 uint64).
void rn_rng_next(void* state, void* out, hipStream_t st);
void rn_add(const void* a, const void* b, void* y, long n, int relu, hipStream_t st);
// part: workspace of >= (rn_bias_act_grad_splits + RN_COLRED_S) * N floats.  db (fp32) / db16 (bf16) written
// (accum: added into) if want_bias; either may be null.  ld: the row stride of dy, h and dh in elements (>= N).
void rn_bias_act_grad(const void* dy, const void* h, void* dh, float* db, void* db16, float* part, int M, int N,
                      long ld, int act, int want_bias, int accum, hipStream_t st);
int rn_bias_act_grad_splits(int M, int N);
// out16[c] (+)= Σ_r in[r][c] for an fp32 [R][C] partial matrix (tmp: rn_colsum_ws(C) floats).
void rn_colsum_f32(const float* in, int R, int C, float* tmp, void* out16, int accum, hipStream_t st);
int rn_colsum_ws(int C);

// ------------------------------------------------------------------ softmax_xent.hip
void rn_softmax_fwd(const void* x, void* y, int M, int N, float scale, hipStream_t st);
void rn_softmax_bwd(const void* dy, const void* y, void* dx, int M, int N, float scale, hipStream_t st);
// loss, lse: M floats; write_grad: the logits are overwritten with their gradient
void rn_xent_fwd(void* logits, const int64_t* tgt, float* loss, float* lse, int M, int V, int nvalid, long ignore,
                 int write_grad, hipStream_t st);
// the fp8 LM head's loss: rn_xent_fwd with write_grad, the gradient to q8 (uint8 [M][V]) as e5m2 · 2^15;
// -1 if V is outside the row kernel's range (a multiple of 8, <= 65536)
int rn_xent_fwd_q8(void* logits, const int64_t* tgt, float* loss, float* lse, int M, int V, int nvalid, long ignore,
                   void* q8, hipStream_t st);
void rn_xent_bwd(const void* logits, const int64_t* tgt, const float* lse, const float* gscale, void* grad, int M,
                 int V, int nvalid, long ignore, hipStream_t st);

// ------------------------------------------------------------------ layernorm.hip
int rn_ln_nv(int E);
// r (optional): residual added first, the sum also written to h.  q8 / st8 (optional): fused e4m3 output
// with delayed scaling (st8 already rolled by the caller).  -1: E not a multiple of 8 or > 8192.
int rn_ln_fwd(const void* x, const void* r, const void* w, const void* b, void* y, void* h, float* mean,
              float* rstd, int M, int E, float eps, hipStream_t st, void* q8, float* st8);
int rn_ln_bwd_blocks(int M);
// waves of the backward grid
int rn_ln_bwd_waves(int M);
// workspace floats: partial rows [blocks][3E] + the reduction's [RN_COLRED_S][3E] scratch
long rn_ln_bwd_ws(int M, int E);
// ws: rn_ln_bwd_ws(M, E) floats.  dw/db (fp32) and dw16/db16 (bf16) outputs, any may be null.
// dxs16 (optional, bf16, always accumulated into): Σ_rows dx — the bias gradient of the layer
// that produced this LayerNorm's input.
// q8 / q8st (optional): dx also in e5m2 with the consumer's delayed scale (q8st rolled here).
int rn_ln_bwd(const void* dy, const void* gh, const void* h, const void* w, const float* mean, const float* rstd,
              void* dx, float* dw, float* db, void* dw16, void* db16, void* dxs16, float* ws, int M, int E,
              int accum, hipStream_t st, void* q8, float* q8st);

// ------------------------------------------------------------------ embedding_optim.hip
// wpe: optional position table (rows of T tokens); V: rows of wte
void rn_emb_fwd(const int64_t* ids, const void* wte, const void* wpe, void* x, int rows, int T, int E, int V,
                hipStream_t st);
// dwte32: V*E fp32 scratch (zeroed here); dwte: bf16 out; dwpe: bf16 (Tp*E) or null
void rn_emb_bwd(const int64_t* ids, const void* dx, float* dwte32, void* dwte, void* dwpe, int B, int T, int Tp,
                int V, int E, hipStream_t st);
// E % 4 == 0.  gwte (bf16 V×E) and gwpe (bf16 ≥T×E, may be null) are accumulated into; d32 (V·E fp32) and
// owner (V) are persistent scratch left in their initial state.
void rn_emb_bwd_acc(const int64_t* ids, const void* dx, float* d32, unsigned* owner, void* gwte, void* gwpe, int B,
                    int T, int E, int V, hipStream_t st);
// deterministic variant: d64 = persistent zeroed V×E 64-bit scratch
void rn_emb_bwd_acc_det(const int64_t* ids, const void* dx, void* d64, unsigned* owner, void* gwte, void* gwpe, int B,
                        int T, int E, int V, hipStream_t st);
// ViT token join: out[b, 0] = cls + pos[0], out[b, 1 + p] = patch[b, p] + pos[1 + p]
void rn_vit_join_fwd(const void* patch, const void* cls, const void* pos, void* out, int B, int P, int E, hipStream_t st);
// backward: dpatch[b, p] = dx[b, 1 + p]; gpos[t] += Σ_b dx[b, t]; gcls += Σ_b dx[b, 0]
void rn_vit_join_bwd(const void* dx, void* dpatch, void* gcls, void* gpos, int B, int P, int E, hipStream_t st);
int rn_norm_ws_floats();
// normbuf[0] = sum(g^2), normbuf[1] = 0 (skip flag); part: rn_norm_ws_floats() floats
void rn_sumsq(const void* g, long n, int is_bf16, float* part, float* normbuf, hipStream_t st);
// state: >= 8 floats of per-step optimizer state on the device
void rn_opt_prep(float* state, float base_lr, float warmup, float total, float min_ratio, int cosine,
                 float lr_override, float b1, float b2, hipStream_t st);
// wdm: weight-decay mask bytes, one per 64 elements; -1: n not a multiple of 8
int rn_adamw(void* p, float* master, const void* g, int g_bf16, float* m, float* v, const uint8_t* wdm,
             float* state, long n, float b1, float b2, float eps, float wd, float grad_scale, float clip, int sr,
             hipStream_t st);
void rn_sgd(void* p, float* master, const void* g, int g_bf16, float* buf, const uint8_t* wdm, float* state, long n,
            float mom, float wd, int nesterov, float grad_scale, float clip, hipStream_t st);

// ------------------------------------------------------------------ gemm_bf16.hip
// persistent-GEMM schedule knobs (gemm_pk.h).  sched: 1 = dynamic tile queue, 0 = static walk; reserve: CUs a
// cfg-9 launch leaves free for a concurrent collective.  Host-side state read at launch.
void rn_gemm_set_sched(int m);
int rn_gemm_get_sched();
void rn_gemm_set_reserve(int r);
int rn_gemm_get_reserve();
// creates the device's counter-slot pool of the dynamic schedule; -1 if it cannot
int rn_gemm_sched_init(int dev);
// a counter slot for a dynamic launch on `st`, or null (static walk)
int* rn_gemm_sched_slot(int dev, hipStream_t st);
// Workspace floats needed for a split-K launch.
long rn_gemm_ws_floats(int M, int N, int split);
// BM of a tile config; rows of the column-partial matrix a config writes (the table in gemm_plan.h).  `cfg` is
// the config that RAN (gemm_plan.h: gemm_resolve), never a request such as -1.
int rn_gemm_cfg_bm(int cfg);
long rn_gemm_colpart_rows(int cfg, int M);
// C[M,N] = act(alpha · op(A)[M,K] · op(B)[K,N] + bias) + res.
//   trans_a = 0: A stored [M][lda] (K contiguous);   1: A stored [K][lda] (M contiguous)
//   trans_b = 0: B stored [K][ldb] (N contiguous);   1: B stored [N][ldb] (K contiguous)
//   cfg: -1 auto, or a tile config (the list is above the definition);  split: -1 auto, 0/1 none
// Returns 0, or -1 if the shape violates the kernel's alignment rules.
// colpart (optional, act-backward only): [rn_gemm_colpart_rows][N] fp32 per-M-tile column sums of C.
// Returns -3 if the requested config / split cannot produce them (the caller then reduces C itself).
int rn_gemm(const void* A, const void* B, void* C, const void* bias, const void* res, void* pre, float* ws,
            const float* alpha, int M, int N, int K, long lda, long ldb, long ldc, int trans_a, int trans_b, int act,
            int split, int out_f32, int accumulate, int cfg, hipStream_t st, float* colpart);

// ------------------------------------------------------------------ gemm_skinny.hip
// Returns -1 for what this config does not take (gemm_plan.h: gemm_cfg_takes(10, ...)) and for a split
// without a workspace.  ``split``: K ranges (>= 1); each is a multiple of 32 deep.
int rn_gemm_skinny(const void* A, const void* W, void* C, const void* bias, const void* res, void* pre, float* ws,
                   const float* alpha, int M, int N, int K, long lda, long ldw, long ldc, int trans_a, int trans_b,
                   int act, int split, int out_f32, int accumulate, const float* colpart, hipStream_t st);
// Decode step QKV projection with the K|V append fused: out = x·Wᵀ + bias (M <= 64 rows = batch
// rows, one new token each) and its columns >= kv_c0 (keys, values) also written into the KV cache
// at the device-side row kv_pos[0] (kv_per_row 0) or kv_pos[m] of batch row m (kv_per_row 1), in a
// cache of kv_len rows; a position outside [0, kv_len) appends nothing.
int rn_gemm_skinny_kv(const void* x, const void* W, const void* bias, void* C, int M, int N, int K,
                      long ldx, long ldw, long ldc, void* kvd, const int64_t* kv_pos, int kv_per_row,
                      int kv_len, long kv_sb, long kv_row, int kv_c0, hipStream_t st);

// ------------------------------------------------------------------ gemm_conv.hip
// Weight-gradient tile variant (mode 3; M = output channels, N = taps × channels) and its tile shape
int rn_conv_wgrad_variant(int M, int N);
void rn_conv_wgrad_tile(int M, int N, int* bm, int* bn);
// Implicit-GEMM convolution (geometry: ConvGeom, gemm_impl.h); mode 1 fwd, 2 dgrad (stride 1), 3 wgrad.
// Returns 0, or -1 if the geometry is outside the implicit path.
int rn_conv_gemm(int mode, const void* A, const void* B, void* C, const void* bias, float* ws, int M, int N, int K,
                 long lda, long ldb, long ldc, int H, int W, int Cg, int RH, int RW, int KH, int KW, int S, int P,
                 int KC, int BC, long bld, int split, int out_f32, int accumulate, float* colpart,
                 hipStream_t st);

// ------------------------------------------------------------------ conv3x3.hip
// tiles (rows of the statistics partials) of the halo-tile conv for this shape; 0 = not taken (the implicit
// GEMM runs instead)
int rn_conv3x3_tiles(int N, int H, int W);
// in / out NHWC [N][H][W][64], w [64][3][3][64]; dgrad: out = dx from in = dy (w flipped / transposed);
// part: forward statistics [tiles][128] (or null); accumulate: out += result.  Returns -1 if not taken.
int rn_conv3x3(const void* in, const void* w, void* out, float* part, int N, int H, int W, int dgrad, int accumulate,
               hipStream_t st);

// ------------------------------------------------------------------ conv.hip
void rn_im2col(const void* x, void* cols, int N, int H, int W, int C, int KH, int KW, int S, int P, int OH, int OW,
               int Kp, hipStream_t st);
void rn_col2im(const void* dcols, void* dx, int N, int H, int W, int C, int KH, int KW, int S, int P, int OH, int OW,
               int Kp, int accumulate, hipStream_t st);
// idx: one byte per output element (window position of the first maximum); K*K <= 256
void rn_maxpool_fwd(const void* x, void* y, void* idx, int N, int H, int W, int C, int K, int S, int P, int OH,
                    int OW, hipStream_t st);
void rn_maxpool_bwd(const void* gy, const void* idx, void* dx, int N, int H, int W, int C, int K, int S, int P,
                    int OH, int OW, hipStream_t st);
void rn_avgpool_fwd(const void* x, void* y, int N, int HW, int C, hipStream_t st);
void rn_avgpool_bwd(const void* gy, void* dx, int N, int HW, int C, hipStream_t st);
// workspace floats: partials [S][2C] + reduced sums [2C] + the column reduction's scratch
long rn_bn_ws_floats(int M, int C);
// C % 8 == 0 && C <= 2048
int rn_bn_supported(int C);
// res (optional): y = relu(BN(x) + res).  partials (optional): [prows][2C] Σx | Σx² row-block partials
// from x's producer (the implicit-conv GEMM epilogue): only their fixed-order column reduction runs,
// not a statistics pass over x.  mask (optional, with relu): [M·C/8] bytes of relu'(y) bits.
void rn_bn_fwd(const void* x, const void* w, const void* b, float* rmean, float* rvar, void* y, float* mean,
               float* rstd, float* ws, int M, int C, float mom, float eps, int relu, const void* res,
               const float* partials, int prows, void* mask, hipStream_t st);
void rn_bn_eval(const void* x, const void* w, const void* b, const float* rmean, const float* rvar, void* y, int M,
                int C, float eps, int relu, const void* res, hipStream_t st);
// dw/db: bf16 outputs [C] (with `accum` ADDED into them); gres (optional): dy ⊙ relu'(y), the gradient of
// a fused residual input; mask: the forward's relu'(y) bits (relu only)
void rn_bn_bwd(const void* gy, const void* x, const void* mask, const void* w, const float* mean, const float* rstd,
               void* dx, void* dw, void* db, float* ws, int M, int C, int relu, void* gres, int accum,
               hipStream_t st);

// ------------------------------------------------------------------ attention.hip
// strides in elements: [b, t, h] for q, k, v, o ; d is contiguous.  bias (optional): fp32 [bias_b][Tq][Tk]
int rn_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const float* bias, int bias_b,
                const long* strides, int B, int H, int Tq, int Tk, int D, float scale, int causal, float p_drop,
                uint64_t seed, const uint64_t* seed_ptr, hipStream_t st);
// strides: q,k,v,o,do,dq,dk,dv (each b,t,h).  delta: B*H*Tq floats workspace.  bsum (optional): packed-QKV
// bias-gradient partials.  q8 / q8st / q8_only / q8part (rn_attn_q8_part_floats floats): see AttnArgs
// (attention_common.h); -3: the kernels cannot emit e5m2 for this shape.
int rn_attn_bwd(const void* dout, const void* q, const void* k, const void* v, const void* o, const float* lse,
                const float* bias, int bias_b, void* dq, void* dk, void* dv, float* delta, const long* s, int B, int H,
                int Tq, int Tk, int D, float scale, int causal, float p_drop, uint64_t seed, const uint64_t* seed_ptr,
                float* bsum, void* q8, float* q8st, int q8_only, float* q8part, hipStream_t st);
// head dims with an MFMA kernel family (32, 64, 128)
int rn_attn_is_fast(int D);
long rn_attn_q8_part_floats(int B, int H, int Tq, int Tk);

// ------------------------------------------------------------------ attention_decode.hip
// q, o: (B, 1, H, 64); k, v: (B, Tk, H, 64) with the given element strides (unit D stride);
// mask: Tk fp32 additive (or null); lens (with no mask): B per-row key counts, int64 if lens64 else
// int32.  Returns -1 for shapes this kernel does not take.
int rn_attn_decode(const void* q, const void* k, const void* v, const float* mask, const void* lens,
                   int lens64, void* o, int B, int H, int Tk, int D, const long* s, float scale,
                   hipStream_t st);

// ------------------------------------------------------------------ attention_window.hip
// T (1..16) new tokens per batch row against a KV cache, append included: qkv (B, T, 3, H, 64) with the
// element strides qs (batch, token, q|k|v, head), kv (B, L <= 1024, 2, H, 64) with cs (batch, row, k|v,
// head), pos: B first write rows (int64 if pos64 else int32, clamped to [0, L] on the device), o
// (B, T, H, 64) contiguous.  Returns -1 for shapes or strides this kernel does not take.
int rn_attn_window(const void* qkv, void* kv, const void* pos, int pos64, void* o, int B, int T, int H,
                   int L, int D, const long* qs, const long* cs, float scale, hipStream_t st);

// ------------------------------------------------------------------ attention_decode_kv8.hip
// The fp8 (OCP e4m3) KV cache: kv8 (B, L, 2, H, 64) bytes with the BYTE strides cs (batch, row, k|v, head, each a
// multiple of 16), kv_scale (B, L, 2, H) fp32 contiguous, one power-of-two scale per 64-element head row.
// pos: pos_n (1 or B) write rows, int64 if pos64 else int32, clamped to [0, L] on the device.
// One-token attention with the append folded in: qkv (B, 1, 3, H, 64) bf16 with the element strides qs (batch,
// q|k|v, head); the new K / V rows are quantised, written to row pos if pos < L, and the query attends rows
// 0 .. pos-1 plus the new row; o (B, 1, H, 64) contiguous.  L <= 1024.  Returns -1 for what it does not take.
int rn_attn_decode_kv8(const void* qkv, void* kv8, float* kv_scale, const void* pos, int pos64, int pos_n, void* o,
                       int B, int H, int L, int D, const long* qs, const long* cs, float scale, hipStream_t st);
// The prefill's append: kv_new (B, T, 2, H, 64) bf16 with the element strides ns (batch, token, k|v, head); rows
// pos[b] + i < L are quantised and written, the others skipped.  Any L.
int rn_kv8_append(const void* kv_new, void* kv8, float* kv_scale, const void* pos, int pos64, int pos_n, int B, int T,
                  int H, int L, int D, const long* ns, const long* cs, hipStream_t st);

// ------------------------------------------------------------------ attention_decode_prefix.hip
// One-token attention for n samples per prompt over a shared prompt cache, the append folded in: qkv
// (B = G n, 1, 3, H, 64) bf16 with the element strides qs (batch, q|k|v, head); prefix_kv (G, P <= 1024, 2, H, 64),
// read only, strides ps (group, row, k|v, head); prefix_len G row counts (int64 if plen64 else int32, clamped to
// [0, P] on the device); kv (B, L <= 1024, 2, H, 64) each row's own tail, strides cs (batch, row, k|v, head); pos B
// write rows (int64 if pos64, clamped to [0, L]).  Row b = g n + s: the new K / V rows are written to kv[b, pos[b]] if
// pos[b] < L and the query attends prefix rows < prefix_len[g], tail rows < pos[b] and the new row; o (B, 1, H, 64)
// contiguous.  1 <= n <= 64.  ws: rn_attn_prefix_ws_floats(G, n, H, P) fp32 of workspace (the split partials).
// Two launches.  Returns -1 for what it does not take.
long rn_attn_prefix_ws_floats(int G, int n, int H, int P);
int rn_attn_decode_prefix(const void* qkv, const void* prefix_kv, const void* prefix_len, int plen64, void* kv,
                          const void* pos, int pos64, float* ws, void* o, int G, int n, int H, int P, int L, int D,
                          const long* qs, const long* ps, const long* cs, float scale, hipStream_t st);

// ------------------------------------------------------------------ sampling.hip
// logits (B, V) bf16 / fp32 with row stride ld >= V; exactly one of u (B fp32 in [0, 1)) and seed
// (row b draws hash_uniform(*seed, b)); params: 3 fp32 on the device (temperature, top_k, top_p)
// overriding the host values, or null.  tokens (B) int64, kept (B) int32.
int rn_sample_logits(const void* logits, int is_bf16, long ld, int B, int V, float temperature, int top_k,
                     float top_p, const float* params, const float* u, const uint64_t* seed,
                     int64_t* tokens, int* kept, hipStream_t st);

// ------------------------------------------------------------------ spec_verify.hip
// Speculative sampling, verification: target (B, K+1, V) / draft (B, K, V) logits, both bf16 or both
// fp32, with the element strides tld / dld (batch, position; the position stride >= V, the last one
// 1), drafts (B, K) int64 contiguous (a value outside [0, V) is rejected on the device), 1 <= K <= 15.
// u: (B, K+1, 2) fp32 (acceptance draw, resample / bonus draw) or seed (position w = b·(K+1)+i draws
// hash_uniform(*seed, 2w) and (.., 2w + 1)): exactly one; params as for rn_sample_logits.
// cand: B·(K+1) uint32 of workspace; tokens (B, K+1) and matched (B) int64.
int rn_spec_verify(const void* target, const long* tld, const void* draft, const long* dld,
                   const int64_t* drafts, int is_bf16, int B, int K, int V, float temperature, int top_k,
                   float top_p, const float* params, const float* u, const uint64_t* seed, uint32_t* cand,
                   int64_t* tokens, int64_t* matched, hipStream_t st);

// ------------------------------------------------------------------ fp8.hip
// state: 4 floats per tensor [scale, amax, amax the scale came from, -]
// state is (re)initialised here (memset node + 2 kernels): current scaling.
void rn_fp8_quantize(const void* x, long n, void* q, float* state, hipStream_t st);
// One-pass delayed-scaling quantisation; graph-capturable.
void rn_fp8_quantize_delayed(const void* x, long n, void* q, float* state, hipStream_t st);
// Re-quantise every cached fp8 weight (segs: device int64 [nseg][4]).  roll = 0: keep the scales already
// in the slots (rebuilding the cache after a checkpoint load).
void rn_fp8_quant_many(const void* flat, const long* segs, int nseg, long max_n, void* qbuf, int roll,
                       hipStream_t st);
// The delayed-scaling roll alone (for producers that quantise inside their own kernel): e4m3 / e5m2 slot.
void rn_fp8_roll(float* state, hipStream_t st);
void rn_fp8_roll_bf8(float* state, hipStream_t st);
void rn_fp8_dequantize(const void* q, long n, const float* state, void* y, hipStream_t st);
// e5m2 gradient quantisation: delayed (roll + one pass) or, for a slot without a scale yet,
// current scaling (memset + amax + quantise)
void rn_bf8_quantize(const void* x, long n, void* q, float* state, int delayed, hipStream_t st);
void rn_bf8_dequantize(const void* q, long n, const float* state, void* y, hipStream_t st);
// dH = dU ⊙ d in e5m2 (+ column partials [rn_act_mul_bf8_groups][N] of dH when colpart).  N % 8 == 0.
// from_h: d holds the pre-activation h and the kernel takes gelu'(h) itself
int rn_act_mul_bf8_groups(long M, int N);
void rn_act_mul_bf8(const void* du, const void* d, long M, int N, void* q, float* state, int delayed, float* colpart,
                    int from_h, hipStream_t st);
// e4m3(gelu(h)) with the delayed-scaling slot `state` (rolled here, amax recorded); n % 8 == 0
void rn_gelu_q8(const void* h, long n, void* q, float* state, hipStream_t st);
// C[M,N] (bf16) = act(sa·sb · A8[M,K] · B8[N,K]ᵀ + bias) + res ; K % 16 == 0, lda/ldb in bytes % 16 == 0
// q8 / q8st (optional, activation-forward with a saved pre-activation only): also write the output
// in e4m3 for the next fp8 GEMM (q8st rolled here).  alpha_ws: 1 float of scratch.
int rn_gemm_fp8(const void* A8, const void* B8, void* C, const void* bias, const void* res, void* pre,
                const float* sa, const float* sb, float* alpha_ws, int M, int N, int K, long lda, long ldb, long ldc,
                int act, hipStream_t st, void* q8, float* q8st);
// dW[M,N] (+)= sa·sb · Σ_k A8[k][m] · B8[k][n]: the fp8 weight gradient, both operands token-major
// (A8 = dY [K][lda] e5m2 if a_bf8 else e4m3, B8 = X [K][ldb] e4m3; lda / ldb in bytes), K = tokens.
// C: bf16 (out_f32 = 0) or fp32, accumulated into when `accumulate`.  ws: rn_gemm_fp8_wgrad_ws floats.
// M, N, lda, ldb multiples of 16, K a multiple of 128.  post (optional device scalar): one more multiplier.
long rn_gemm_fp8_wgrad_split(int M, int N, int K);
long rn_gemm_fp8_wgrad_ws(int M, int N, int K);
int rn_gemm_fp8_wgrad(const void* A8, const void* B8, void* C, const float* sa, const float* sb, float* alpha_ws,
                      float* ws, int M, int N, int K, long lda, long ldb, long ldc, int accumulate, int out_f32,
                      int a_bf8, hipStream_t st, const float* post);
// C[M,N] (bf16) = sa·sb · A8[M][K] · B8[K][N]: the fp8 data gradient dX = dY·W with dY (A8, e5m2 if
// a_bf8) K-contiguous and the weight W [out = K][in = N] as stored, read transposed.  K, N, lda, ldb, ldc
// multiples of 16 (bytes for the fp8 operands).  post (optional device scalar): one more output multiplier.
int rn_gemm_fp8_dgrad(const void* A8, const void* B8, void* C, const float* sa, const float* sb, float* alpha_ws,
                      int M, int N, int K, long lda, long ldb, long ldc, int a_bf8, hipStream_t st, const float* post);

// ------------------------------------------------------------------ comm_proxy.hip
// one-GPU stand-in for a collective's footprint: `wgs` workgroups move volume_bytes through the `bytes`-long
// bucket buf (values unchanged), paced to gbps GB/s in total
void rn_comm_proxy(void* buf, long bytes, double volume_bytes, int wgs, double gbps, hipStream_t st);

}  // extern "C"
