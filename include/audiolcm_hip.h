/*
 * audiolcm_hip.h — C-ABI of libaudiolcm_hip.so, the MI355X (gfx950) hot path of
 * AudioLCM text-to-audio inference.
 *
 * Conventions:
 *   - every entry point is `extern "C" int fn(...)`: 0 on success, a negative
 *     ALCM_E* code otherwise; alcm_last_error() returns a thread-local message;
 *   - every tensor argument is a caller-allocated DEVICE pointer (typically a
 *     torch tensor's data_ptr()) in the reference's own layout unless stated,
 *     fp32, contiguous; sizes are explicit;
 *   - work is enqueued on the caller's hipStream_t (torch.cuda.current_stream());
 *     no call allocates device memory except the *_create loaders, no call
 *     synchronises the host;
 *   - concurrency: calls on one model handle from different host threads and/or
 *     different caller streams may overlap, provided each concurrent call has its
 *     own workspace and output buffers.  The handle's packed weights are read-only
 *     after *_create; the only per-handle mutable state is the set of auxiliary
 *     streams/events alcm_bigvgan_forward forks its resblock chains onto, which is
 *     kept per CALLER stream (created under a lock on that stream's first call), so
 *     concurrent calls never share an event.  alcm_model_set_precision /
 *     alcm_model_set_resblock_streams must not race with calls on the same handle.
 *     Two calls on the SAME caller stream are ordered by that stream;
 *   - no torch types cross the boundary.
 *
 * Reference interfaces replaced (paths under the reference checkout):
 *   alcm_dit_*          ConcatDiT2MLP.forward          ldm/modules/diffusionmodules/concatDiT.py:282-304
 *                       (called as LCM_audio.apply_model, ldm/models/diffusion/lcm_audio.py:479-502)
 *   alcm_lcm_step       LCMSampler.step (eps branch)   ldm/models/diffusion/scheduling_lcm.py:410-496
 *   alcm_*_embedding    get_guidance_scale_embedding   scheduling_lcm.py:87-113
 *                       TimestepEmbedder.timestep_embedding  concatDiT.py:49-67
 *   alcm_vae_*          LCM_audio.decode_first_stage   lcm_audio.py:392-406 -> AutoencoderKL.decode
 *                       autoencoder1d.py:59-62, Decoder1D.forward autoencoder1d.py:484-517
 *   alcm_bigvgan_*      BigVGAN.forward                vocoder/bigvgan/models.py:181-203
 *                       (VocoderBigVGAN.vocode, models.py:406-411)
 *   alcm_activation1d   Activation1d.forward           vocoder/bigvgan/alias_free_torch/act.py:23-27
 *   alcm_gemm           aten conv1d / conv_transpose1d / linear / bmm on the path (SURVEY.md §2 kernel inventory)
 */
#ifndef AUDIOLCM_HIP_H
#define AUDIOLCM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* alcm_stream_t; /* hipStream_t */

enum {
  ALCM_OK = 0,
  ALCM_E_INVALID = -1,  /* bad argument / shape */
  ALCM_E_HIP = -2,      /* HIP runtime error */
  ALCM_E_MISSING = -3,  /* required weight tensor missing */
  ALCM_E_WORKSPACE = -4 /* workspace too small */
};

/* ---------------------------------------------------------------- misc */
const char* alcm_last_error(void);
int alcm_version(void);
/* device properties check: returns 0 if device `dev` is gfx950 */
int alcm_check_device(int dev);

/* ---------------------------------------------------------------- generic MFMA GEMM / implicit-GEMM conv1d
 * C[m][n] = epilogue( sum_k A[m][k] * B[n][k] ), MFMA with fp32 accumulate.  Operand precision `prec`:
 *   ALCM_PREC_BF16  (0) one v_mfma_f32_16x16x32_bf16 (operands rounded to bf16)
 *   ALCM_PREC_SPLIT (1) 3-term bf16 split (hi*hi + hi*lo + lo*hi): fp32-level accuracy, 3x the MFMA work
 *   ALCM_PREC_F16   (2) one v_mfma_f32_16x16x32_f16 (operands rounded to fp16)
 *   ALCM_PREC_F16W2 (3) fp16 activation x fp16 hi+lo weight, 2 MFMAs (alcm_opconv only) */
enum { ALCM_PREC_BF16 = 0, ALCM_PREC_SPLIT = 1, ALCM_PREC_F16 = 2, ALCM_PREC_F16W2 = 3 };
enum { ALCM_OPND_ACT = 0, ALCM_OPND_ACT_T = 1, ALCM_OPND_WEIGHT = 2 };

typedef struct alcm_operand {
  int kind;
  const void* ptr;
  /* ACT: element (b, t, c) at ptr + b*sb + t*st + c*sc; K index k = tap*Cpad + ci, source time
   *      t_src = t + tap*dil - pad (up == 2: nearest-x2 upsampled input, t_up = t + tap*dil - pad,
   *      t_src = t_up/2, valid for t_up in [0, 2*T_in)), zero outside [0, T_in) / ci >= C_in / k >= ksize*Cpad.
   *      With C_in < Cpad (the scalar loader) the zero of the lanes ci >= C_in is the WEIGHT operand's: a norm
   *      prologue leaves (0 - mean)*rstd in those lanes of A, and alcm_pack_conv_weight writes exact zeros at
   *      ci >= C_in of every tap, so the product is the defined one.  A WEIGHT operand packed any other way must keep
   *      those columns zero (tests/test_gpu_gemm_forms.py, case ln_k9_C20: rows of mean ~ 5 std).
   * ACT_T: element (n, k) at ptr + k*st + n*sc, valid k < T_in, n < rows.
   * WEIGHT: packed [rows][Kpad] planes: bf16 hi at ptr, bf16 lo at ptr + w_lo_off, fp16 hi at
 *         ptr + 2*w_lo_off, fp16 lo at ptr + 3*w_lo_off (elements; w_lo_off = rows*Kpad as written by
 *         alcm_pack_conv_weight). */
  int64_t sb, st, sc;
  int T_in, C_in, Cpad, ksize, dil, pad, up;
  int rows_per_batch; /* ACT: rows m -> (b = m / rows_per_batch, t = m % rows_per_batch) */
  int rows;           /* ACT_T / WEIGHT: number of valid rows */
  int64_t zs1, zs2;   /* batched offset (z / zdiv)*zs1 + (z % zdiv)*zs2 */
  /* ACT prologue, applied to valid (non-padding) elements: v = (v - mean[b*T_in+t_src]) * rstd[...]
   * (if pro_mean), v = v*pro_scale[b*pro_sb+c] + pro_shift[...] (if pro_scale), v = act(v)
   * with pro_act 0 (none) or 1 (SiLU); other codes are rejected with ALCM_E_INVALID */
  const float* pro_scale;
  const float* pro_shift;
  int64_t pro_sb;
  const float* pro_mean;
  const float* pro_rstd;
  int pro_act;
  int64_t w_lo_off;
} alcm_operand;

typedef struct alcm_gemm_args {
  int M, N, Kpad; /* Kpad: multiple of 32 covering the real K */
  int batch, zdiv;
  alcm_operand a, b;
  /* activation codes: 0 none, 1 SiLU, 2 GELU (erf), 3 GELU (tanh), 4 tanh
   * epilogue: v = acc*acc_scale + bias[n]; v = act(v) (geglu 1: v_even * gelu_erf(v_odd) -> column n/2,
 *           geglu 2: v_even * gelu_tanh(v_odd), T5's gated-gelu with (wi_1, wi_0) rows interleaved);
   *           v += res[...]; v *= out_scale; if accumulate v += out[...]; out[...] = v
   * output row m -> (b, t), stored at out + zoff + b*o_sb + (t*out_step + out_off)*o_st + n*o_sc */
  const float* bias;
  float acc_scale, out_scale;
  int act, accumulate, geglu;
  const float* res;
  int64_t r_sb, r_st, r_sc, r_zs1, r_zs2;
  float* out;
  int64_t o_sb, o_st, o_sc, o_zs1, o_zs2;
  int out_rows_per_batch, out_step, out_off;
  int prec;           /* ALCM_PREC_* */
  int disable_window; /* 1: never use the window-conv kernel (testing / A-B timing) */
  int tile_n;         /* 0: automatic; 64 / 128: force the N tile of the window-conv kernel */
} alcm_gemm_args;

int alcm_gemm(const alcm_gemm_args* args, alcm_stream_t stream);

/* pack a conv/linear weight W[co][ci][k] (fp32, DEVICE) into four [Cout][Kpad] planes (bf16 hi, bf16 lo,
 * fp16 hi, fp16 lo) with K index = tap*Cpad + ci. transposed=1 takes a ConvTranspose1d weight [ci][co][k]
 * and a phase (stride s, phase r) selecting taps j = r + s*(Q-1-tap), Q = k/s. out must hold 4*Cout*Kpad u16. */
int alcm_pack_conv_weight(const float* w, int c_out, int c_in, int k, int cpad, int kpad, int transposed,
                          int stride, int phase, void* out, alcm_stream_t stream);

/* ---------------------------------------------------------------- normalisation / elementwise
 * Layout of x for the norm kernels: element (b, t, c) at x + b*sb + t*st + c (channels contiguous). */
int alcm_group_norm_affine(const float* x, int B, int T, int C, int64_t sb, int64_t st, int groups,
                           float eps, const float* gamma, const float* beta, float* scale_out,
                           float* shift_out, alcm_stream_t stream);
int alcm_row_stats(const float* x, int rows, int C, int64_t ld, float eps, float* mean, float* rstd,
                   alcm_stream_t stream);
int alcm_layer_norm(const float* x, int rows, int C, int64_t ld_in, float eps, const float* gamma,
                    const float* beta, const float* add, int64_t ld_add, float* y, int64_t ld_out,
                    alcm_stream_t stream);
int alcm_softmax_rows(float* x, int rows, int n, int64_t ld, alcm_stream_t stream);
/* LayerNorm of rows (row stride ld) written as an MFMA operand plane [rows][C] (prec PREC_F16 (2) or
 * PREC_BF16 (0)) for alcm_opconv (the DiT feed-forward input, concatDiT.py:120-125) */
int alcm_layer_norm_plane(const float* x, int rows, int C, int64_t ld, float eps, const float* gamma,
                          const float* beta, void* plane, int prec, alcm_stream_t stream);
/* fused Activation1d(SnakeBeta): x,y DEVICE (b,t,c) channels-last, not in place; alpha_exp = exp(alpha),
 * inv_beta = 1/(exp(beta)+1e-9) per channel (DEVICE); up_filter/down_filter: HOST arrays of 12 taps */
int alcm_activation1d(const float* x, float* y, int B, int T, int C, int64_t sb, int64_t st,
                      const float* alpha_exp, const float* inv_beta, const float* up_filter,
                      const float* down_filter, alcm_stream_t stream);

/* ---------------------------------------------------------------- operand-format AMPBlock path
 * (vocoder/bigvgan/models.py:72-81 as Activation1d -> conv, alcm_opconv.hip)
 * alcm_activation1d_op: Activation1d of x (B,T,C) fp32 channels-last DEVICE into MFMA operand planes
 *   y [B][T][Cp] of 2-byte elements (Cp = multiple of 32 >= C, channels >= C written as 0): prec
 *   ALCM_PREC_F16 / F16W2 -> one fp16 plane; BF16 -> one bf16 plane; SPLIT -> bf16 hi plane at y and
 *   bf16 lo plane at y + B*T*Cp.  alpha_exp / inv_beta DEVICE, filters HOST (12 taps). */
int alcm_activation1d_op(const float* x, void* y, int B, int T, int C, int Cp, const float* alpha_exp,
                         const float* inv_beta, const float* up_filter, const float* down_filter, int prec,
                         alcm_stream_t stream);
/* alcm_activation1d_op_f16in: alcm_activation1d_op (alias_free_torch/act.py:23-27) of an fp16 plane x16 [B][T][C]
 *   DEVICE — the BigVGAN AMPBlock conv1 output written by alcm_opconv's out_plane epilogue (vocoder/bigvgan/
 *   models.py:74-79: that conv's only consumer is this activation) — into fp16 planes y [B][T][C].  Only the shapes
 *   whose FIR input alcm_activation1d_op rounds to fp16 anyway: prec ALCM_PREC_F16, C >= 192, C % 64 == 0, Cp == C,
 *   16-byte aligned x16 / y; the result equals alcm_activation1d_op on the fp32 conv output bit for bit.
 *   ALCM_E_INVALID otherwise. */
int alcm_activation1d_op_f16in(const void* x16, void* y, int B, int T, int C, int Cp, const float* alpha_exp,
                               const float* inv_beta, const float* up_filter, const float* down_filter, int prec,
                               alcm_stream_t stream);
/* alcm_activation1d_planes: the general form of the two entries above, which are its nset = 1 cases.  x: (B,T,C) fp32,
 *   or with x_is_f16 an fp16 plane [B][T][C] (alcm_activation1d_op_f16in's shapes only); nset = 1, or 3 for three
 *   Activation1d of the one input with their own SnakeBeta parameters and the same FIR taps (a BigVGAN stage's three
 *   resblocks' first half-layer) in one pass: planes y[i] from alpha_exp[i] / inv_beta[i], i < nset, bit-identical to
 *   nset single calls.  Zero-initialise the struct before setting fields. */
typedef struct alcm_act_args {
  const void* x;
  int x_is_f16;
  void* y[3];
  int nset;
  int B, T, C, Cp;
  const float* alpha_exp[3];
  const float* inv_beta[3];
  const float* up_filter;   /* HOST, 12 taps */
  const float* down_filter; /* HOST, 12 taps */
  int prec;
} alcm_act_args;
int alcm_activation1d_planes(const alcm_act_args* args, alcm_stream_t stream);
/* alcm_opconv: out (B,T,N) = conv_{ksize,dil}(a) with same-length zero padding (2*pad == (ksize-1)*dil)
 * on operand planes a (as written by alcm_activation1d_op, lo plane a_lo_off elements after hi), weights
 * packed by alcm_pack_conv_weight with cpad = Cp; epilogue as alcm_gemm: v = acc + bias[n];
 * v = act(v); v += res; v *= out_scale; if accumulate v += out.  prec: BF16 / SPLIT / F16 / F16W2
 * (must match the planes a holds); C = real input channels (cost accounting). */
/* Zero-initialise the whole struct (memset / `= {0}`) before setting fields: optional trailing fields (act_*, geglu_plane,
 * out_stride / out_offset / out_rows, out_plane) are read as "off" only when zero, and later versions append more. */
typedef struct alcm_opconv_args {
  const void* a;
  int64_t a_lo_off;
  int B, T, C, Cp;
  int ksize, dil, pad;
  const void* w;
  int64_t w_lo_off;
  int kpad, N;
  const float* bias;
  const float* res;
  float* out;
  int out_act, accumulate;
  float out_scale;
  int prec;
  /* optional fused Activation1d epilogue (alias_free_torch/act.py:23-27 applied to v = conv + bias (+ res)):
   * when act_plane != NULL the kernel also writes Activation1d(v) as MFMA operand planes [B][T][Cp'] with
   * Cp' = round_up(N, 32), in the format `prec` reads (SPLIT: lo plane act_plane_lo_off elements after hi),
   * ready for the next conv.  `out` may then be NULL (no fp32 output).  Tiles recompute 8 halo rows, so
   * `out` must not overlap `res`.  alpha_exp / inv_beta are device arrays of N (exp(alpha),
   * 1/(exp(beta)+1e-9)); the 12-tap filters are HOST arrays.  Requires out_act == 0 and N even. */
  void* act_plane;
  int64_t act_plane_lo_off;
  const float* act_alpha_exp;
  const float* act_inv_beta;
  const float* act_up_filter;
  const float* act_down_filter;
  /* optional GEGLU epilogue (new_attention.py:48-55 with value/gate rows interleaved: output columns 2j, 2j+1
   * = value j, gate j): when geglu_plane != NULL the kernel writes (v_2j + b_2j) * gelu_erf(v_2j+1 + b_2j+1)
   * as an operand plane [B][T][N/2] in the format of `prec` (F16 / BF16) instead of the fp32 output; needs
   * res == NULL, out_act == 0 and the wide-layer kernel (N % 128 == 0, Cp % 64 == 0). */
  void* geglu_plane;
  /* optional strided output (one phase of a ConvTranspose1d, vocoder/bigvgan/models.py:160-165): when
   * out_stride > 0, output row t of batch b is row t * out_stride + out_offset of an fp32 [B][out_rows][N]
   * `out`, and `pad` may be any value in [0, (ksize-1)*dil] (input row t - pad + tap*dil, zero outside).
   * Needs F16/BF16, N % 192 == 0, Cp % 64 == 0 and no res / accumulate / out_act / act / GEGLU.
   * 0 (the zero-initialised default): same-length conv, out is [B][T][N]. */
  int out_stride, out_offset, out_rows;
  /* optional operand-plane output: when out_plane != NULL the kernel writes conv + bias as an F16 / BF16 plane
   * [B][T][N] (the format of `prec`) instead of the fp32 `out` (which may be NULL) — for a consumer that rounds to
   * that format anyway (the DiT q/k/v projection feeding the fused attention).  Needs the wide-layer kernel
   * (F16 / BF16, N % 4 == 0, Cp % 64 == 0) and no res / accumulate / out_act / act / GEGLU / strided output. */
  void* out_plane;
  /* optional K-split workspace (fp32, 16-byte aligned, ksplit_ws_floats floats): where the persistent wide-layer
   * kernel's grid would not fill the chip (the DiT FFN down-projection: 192 tiles of 256 x 192 on 256 CUs), the
   * library may split the 64-channel K chunks into P parts (P * B * T * N <= ksplit_ws_floats), write P fp32
   * partial slices here and reduce them in part order with the bias / residual / scale / accumulate epilogue (a
   * second launch on the same stream): deterministic, not bit-identical to the unsplit sum.  NULL: never split. */
  float* ksplit_ws;
  int64_t ksplit_ws_floats;
} alcm_opconv_args;
int alcm_opconv(const alcm_opconv_args* args, alcm_stream_t stream);
/* alcm_opconv_sum: out = (sum over i < n of conv_i(args[i].a) + args[i].bias + args[i].res) * args[0].out_scale
 *   (+ out when args[0].accumulate), 1 <= n <= 3 — the mean over a BigVGAN stage's resblocks (vocoder/bigvgan/
 *   models.py:190-199: xs += resblock_j(x); x = xs / num_kernels) taken at the chains' last conv2 + residual
 *   (models.py:76-80), so the stage output is written once instead of read and rewritten per chain.  Each term is
 *   an alcm_opconv same-length conv with its own planes, weights, ksize / pad, bias and residual; the terms share B,
 *   T and N, and only args[0]'s out / out_scale / accumulate are read (another term's out must be NULL or the same).
 *   Three F16 / BF16 terms of dilation 1 with Cp % 64 == 0 and N % 192 == 0 run as one launch summing all taps in one
 *   fp32 accumulator; otherwise the terms run in order, each accumulating into out (the same value up to fp32
 *   rounding order).  No activation / plane / GEGLU / strided outputs.  Every term passes alcm_opconv's operand
 *   checks before anything is launched, in either form (ALCM_E_INVALID otherwise). */
int alcm_opconv_sum(const alcm_opconv_args* args, int n, alcm_stream_t stream);
/* alcm_opconv_dense: the narrow AMPBlock conv of BigVGAN stages 3-5 (vocoder/bigvgan/models.py:72-81, C = N in
 * {24, 48} at F16 / F16W2, 96 at F16; ksize <= 11, (ksize-1)*dil <= 64) with the weights resident in LDS: same
 * arguments as alcm_opconv except that w is packed by alcm_pack_conv_weight with cpad = C (dense K = tap*C + c,
 * kpad = round_up(ksize*C, 32)); the planes a may be wider (Cp > C: channels >= C are ignored) and the fused
 * Activation1d writes only channels < N of its planes.  Epilogues: act (conv1), res + out + act (conv2), res + out
 * with out_scale and accumulate, no act (a resblock's last conv2).  ALCM_E_INVALID for anything else. */
int alcm_opconv_dense(const alcm_opconv_args* args, alcm_stream_t stream);

/* alcm_flash_attention: multi-head self-attention of the DiT (CrossAttention with context = x,
 * ldm/modules/new_attention.py:89-130, the q/k/v projections already applied):
 * out[b, i, h*dh:(h+1)*dh] = softmax_j(q_i . k_j * dh^-1/2) v_j per head, scores kept on chip.
 * qkv: (B, L, 3H) fp32 DEVICE rows [q | k | v] (16-byte aligned), out: (B, L, H) fp32; dh = H / heads <= 72;
 * prec: ALCM PREC_F16 (2) or PREC_BF16 (0) operand rounding of q, k, v and the probabilities. */
int alcm_flash_attention(const float* qkv, float* out, int B, int L, int H, int heads, int prec, alcm_stream_t stream);
/* alcm_flash_attention_ex: the same fused attention with every form the models launch — the DiT self-attention
 * (ldm/modules/new_attention.py:89-130) and, inside FrozenCLAPFLANEmbedder.encode (ldm/modules/encoders/modules.py:
 * 567-582), HF BertSelfAttention (no bias, dh^-1/2) and HF T5Attention (position bias, unscaled scores):
 * out[b, i, h*dh:(h+1)*dh] = softmax_j(scale * q_i . k_j + bias[h][i][j]) v_j.
 *   input, exactly one of: qkv (B, L, 3H) fp32 rows (16-byte aligned), or qkv_plane (B, L, 3H) rows of 2-byte operand
 *     elements in the format of prec (row pitch 3H, 8-byte aligned, L <= 512);
 *   output: out_plane != NULL: (B, L, H) rows of 2-byte elements in the format of prec (row pitch H, the result
 *     rounded once more), out is not written; otherwise out (B, L, H) fp32;
 *   bias: NULL, or fp32 [heads][bld][bld] with bld >= L, element (h, i, j) added to the score of query i and key j
 *     (L <= 512); scale: 0 = dh^-1/2, > 0 replaces it (L <= 512).
 * dh = H / heads <= 72, dh % 4 == 0; prec ALCM_PREC_F16 (2) or ALCM_PREC_BF16 (0).  ALCM_E_INVALID otherwise. */
int alcm_flash_attention_ex(const float* qkv, const void* qkv_plane, float* out, void* out_plane, int B, int L, int H,
                            int heads, int prec, const float* bias, int bld, float scale, alcm_stream_t stream);
/* the arguments of alcm_flash_attention_ex as a struct (alcm_debug_attn_plan) */
typedef struct alcm_attn_args {
  const float* qkv;
  const void* qkv_plane;
  float* out;
  void* out_plane;
  int B, L, H, heads, prec;
  const float* bias;
  int bld;
  float scale;
} alcm_attn_args;
/* alcm_softmax_rows_bias: in-place softmax of HF T5Attention's scores + position_bias (the split-policy text
 * tower of FrozenCLAPFLANEmbedder.encode, ldm/modules/encoders/modules.py:567-582): rows = Z*L rows of pitch ld,
 * row r = (z, i) with i = r % L, head h = z % heads: x[r][j] = softmax_j(x[r][j] + bias[(h*bld + i)*bld + j]) for
 * j < n, and x[r][n..ld) = 0 (the K padding the P.V GEMM reads).  bld >= max(n, L), ld >= n. */
int alcm_softmax_rows_bias(float* x, int rows, int n, int64_t ld, int L, int heads, const float* bias, int bld,
                           alcm_stream_t stream);

/* ---------------------------------------------------------------- LCM scheduler pieces */
/* coeffs (HOST array of 6): {sqrt_a, sqrt_b, c_out, c_skip, sqrt_a_prev, sqrt_b_prev};
 * noise may be NULL (final step: prev_out = denoised) */
int alcm_lcm_step(const float* x, const float* eps, const float* noise, const float* coeffs,
                  float* prev_out, float* denoised_out, int64_t n, alcm_stream_t stream);
/* classifier-free-guidance variant (config 4): eps = eps_uncond + cfg_scale*(eps_cond - eps_uncond)
 * (plms.py:184-186 / ddim.py:203-205) fused into the same step */
int alcm_lcm_step_cfg(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                      const float* noise, const float* coeffs, float* prev_out, float* denoised_out, int64_t n,
                      alcm_stream_t stream);
/* alcm_lcm_step_edit: the step above (eps_uncond may be NULL: no guidance combine) on (B, C, T) latents with a known
 * latent z0 (B, C, T) blended in per frame by mask (B, T) in [0, 1], 1 = regenerate:
 *   d' = m * d + (1 - m) * z0   (d: the step's denoised value; m = 1 gives d and m = 0 gives z0, bit for bit)
 *   denoised_out = d',  prev_out = noise ? sqrt_a_prev * d' + sqrt_b_prev * noise : d'.
 * 16-byte accesses along T when T % 4 == 0 and every pointer is 16-byte aligned, element accesses otherwise.
 * ALCM_E_INVALID for a null x, eps_cond, coeffs, z0 or mask, both outputs null, or a negative B, C or T. */
int alcm_lcm_step_edit(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                       const float* noise, const float* coeffs, const float* z0, const float* mask, float* prev_out,
                       float* denoised_out, int B, int C, int T, alcm_stream_t stream);
/* alcm_lcm_step_joint: the step above (LCMSampler.step, scheduling_lcm.py:465-486; eps_uncond may be NULL: no guidance
 * combine) on one long latent whose overlapping windows went through the DiT as one batch (no reference counterpart:
 * the reference generates one window).
 *   x, noise, prev_out, denoised_out (B, C, L); eps_cond, eps_uncond, xw_out (K * B, C, W), row k * B + b: window k of
 *   clip b, frames starts[k] .. starts[k] + W of the long latent; starts: HOST array of K ints; wn (K, W), device: the
 *   normalised window weights (audiolcm_amd/pipeline.py joint_weights: per frame the covering windows' weights sum
 *   to 1, and a frame under one window has weight exactly 1).
 *   Per element (b, c, t), over the windows covering t in ascending k: d_k = the step's denoised value from x[b, c, t]
 *   and eps[k * B + b, c, t - starts[k]].  One covering window: d = d_k, alcm_lcm_step's bits.  Several:
 *   acc = wn[k0] * d_k0 (rounded alone), acc = fmaf(wn[k], d_k, acc) for the further ones, d = acc.
 *   denoised_out = d,  prev_out = noise ? sqrt_a_prev * d + sqrt_b_prev * noise : d,
 *   xw_out[k * B + b, c, t - starts[k]] = prev for every covering k (the next DiT input).
 * Any output may be NULL, not all three.  eps_cond NULL: x itself is gathered into xw_out (the first DiT input);
 * eps_uncond, noise, prev_out and denoised_out must then be NULL.  No atomics: an element's bits do not depend on B,
 * the grid or the access width.  16-byte accesses when L, W and every start are multiples of 4 and every pointer is
 * 16-byte aligned, element accesses otherwise.
 * ALCM_E_INVALID for a null x, wn, coeffs or starts, no output, a negative B, C, L or W, K outside 1 .. 32, or starts that
 * do not begin at 0, do not ascend strictly, leave a gap (starts[k] > starts[k - 1] + W) or do not end at L
 * (starts[K - 1] + W != L).  B, C, L or W of 0: no launch. */
int alcm_lcm_step_joint(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                        const float* noise, const float* coeffs, const int* starts, int K, const float* wn,
                        float* prev_out, float* denoised_out, float* xw_out, int B, int C, int L, int W,
                        alcm_stream_t stream);
/* alcm_lcm_step_joint_edit: alcm_lcm_step_joint with a known latent blended in, as alcm_lcm_step_edit does for one
 * window (joint inpainting, variation and extension of a recording; the same kernel body).  The arguments are
 * alcm_lcm_step_joint's plus z0 (B, C, L) and mask (B, L) in [0, 1], 1 = regenerate.  Per element (b, c, t):
 *   d  = alcm_lcm_step_joint's value, bit for bit (one covering window: alcm_lcm_step's bits; several: the first
 *        product rounded alone, fmaf for the further ones in ascending k);
 *   d' = m * d + (1 - m) * z0[b, c, t] with m = mask[b, t]  (m = 1 gives d and m = 0 gives z0, bit for bit);
 *   denoised_out = d',  prev_out = noise ? sqrt_a_prev * d' + sqrt_b_prev * noise : d',
 *   xw_out[k * B + b, c, t - starts[k]] = prev for every covering k.
 * With one window (K = 1) prev_out and denoised_out are alcm_lcm_step_edit's bits.  Any output may be NULL, not all
 * three.  There is no gather-only form: the first DiT input comes from alcm_lcm_step_joint with eps_cond = NULL.  No
 * atomics: an element's bits do not depend on B, the grid or the access width.  16-byte accesses under
 * alcm_lcm_step_joint's conditions with z0 and mask 16-byte aligned too, element accesses otherwise.
 * ALCM_E_INVALID for everything alcm_lcm_step_joint refuses and for a null eps_cond, z0 or mask.  B, C, L or W of 0: no
 * launch.  The ring's form is alcm_lcm_step_ring_edit. */
int alcm_lcm_step_joint_edit(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                             const float* noise, const float* coeffs, const int* starts, int K, const float* wn,
                             const float* z0, const float* mask, float* prev_out, float* denoised_out,
                             float* xw_out, int B, int C, int L, int W, alcm_stream_t stream);
/* alcm_lcm_step_ring: alcm_lcm_step_joint on a ring of L frames instead of a line (seamless loops; the same kernel
 * body).  Arguments, outputs and the eps-less gather form are alcm_lcm_step_joint's.  Window k covers frame t at the
 * offset o = t - starts[k], plus L when that is negative, if o < W; eps and xw_out are read and written at that offset,
 * and wn is audiolcm_amd/pipeline.py ring_weights.  Per element the chain over the covering windows in ascending k is
 * the open entry's: one covering window gives alcm_lcm_step's bits, several the first product rounded alone and fmaf
 * for the further ones.  16-byte accesses under the open entry's conditions; an access then never straddles the wrap.
 * ALCM_E_INVALID as for alcm_lcm_step_joint, except for the plan: K outside 2 .. 32, W > L, starts that do not begin at
 * 0, do not ascend strictly, reach L (starts[K - 1] >= L) or leave a gap (starts[k] > starts[k - 1] + W, or
 * starts[K - 1] + W < L). */
int alcm_lcm_step_ring(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                       const float* noise, const float* coeffs, const int* starts, int K, const float* wn,
                       float* prev_out, float* denoised_out, float* xw_out, int B, int C, int L, int W,
                       alcm_stream_t stream);
/* alcm_lcm_step_ring_edit: alcm_lcm_step_ring with a known latent blended in, as alcm_lcm_step_joint_edit does on a
 * line (a loop made from a recording; the same kernel body; no reference counterpart: the reference generates one
 * window, LCMSampler.step, scheduling_lcm.py:465-486).  The arguments are alcm_lcm_step_ring's plus z0 (B, C, L) and
 * mask (B, L) in [0, 1], 1 = regenerate.  Per element (b, c, t):
 *   d  = alcm_lcm_step_ring's value, bit for bit (offsets modulo L, the chain over the covering windows in ascending k,
 *        wn the ring's table);
 *   d' = m * d + (1 - m) * z0[b, c, t] with m = mask[b, t]  (m = 1 gives d and m = 0 gives z0, bit for bit);
 *   denoised_out = d',  prev_out = noise ? sqrt_a_prev * d' + sqrt_b_prev * noise : d',
 *   xw_out = prev gathered with the wrap: at the offset (t - starts[k]) mod L of every covering window k.
 * On a plan no window of which wraps (starts[K - 1] + W == L) the outputs are alcm_lcm_step_joint_edit's bits.  Any
 * output may be NULL, not all three.  There is no gather-only form: the first DiT input comes from alcm_lcm_step_ring
 * with eps_cond = NULL.  16-byte accesses under alcm_lcm_step_ring's conditions with z0 and mask 16-byte aligned too.
 * ALCM_E_INVALID for everything alcm_lcm_step_ring refuses and for a null eps_cond, z0 or mask.  B, C, L or W of 0: no
 * launch. */
int alcm_lcm_step_ring_edit(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                            const float* noise, const float* coeffs, const int* starts, int K, const float* wn,
                            const float* z0, const float* mask, float* prev_out, float* denoised_out, float* xw_out,
                            int B, int C, int L, int W, alcm_stream_t stream);
/* alcm_wave_loop: one period of a looping clip cut from a longer decode of the same ring, with the seam closed, one
 * launch (no reference counterpart).
 *   ext (B, row_len): the decode of the ring's latent padded circularly; out (B, N); ramp (R entries, device):
 *   alcm_wave_paste's fade table, ramp[0] = 1.
 *   out[n] = ext[start + n] for n >= R, bit for bit;
 *   out[0] = ext[start + N] bit for bit (R >= 1): the sample that follows out[N - 1] in ext;
 *   out[n] = fmaf(ramp[n], ext[start + N + n] - ext[start + n], ext[start + n]) for 0 < n < R.
 * R = 0 is a plain crop.  out must not overlap ext.  16-byte accesses when start, N and row_len are multiples of 4 and
 * ext and out are 16-byte aligned, element accesses otherwise.
 * ALCM_E_INVALID for a null ext or out (ramp with R > 1), a negative size or start, R > N, or start + N + R > row_len.
 * B or N of 0: no launch. */
int alcm_wave_loop(const float* ext, const float* ramp, float* out, int B, int64_t row_len, int64_t start, int64_t N,
                   int R, alcm_stream_t stream);
/* alcm_latent_init: the encoder output (or a given latent) -> the edit sampler's starting point, one launch.
 *   exactly one of moments (B, 2C, T: mean | logvar, AutoencoderKL.encode) and z0_in (B, C, T);
 *   z0 = z0_in, or scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * e0); e0 (B, C, T) NULL: the posterior mode
 *        scale * mean (e0 is ignored with z0_in);
 *   x  = m * (sa_r * z0 + sb_r * noise) + (1 - m) * (sa * z0 + sb * noise), m = mask[b][t] (B, T);
 *        mask NULL: x = sa * z0 + sb * noise.
 * z0_out / x_out (B, C, T): either may be NULL, not both; noise (B, C, T) is needed for x_out.  ALCM_E_INVALID
 * otherwise, or for a negative B, C or T. */
int alcm_latent_init(const float* moments, const float* z0_in, const float* e0, float scale, const float* noise,
                     const float* mask, float sa, float sb, float sa_r, float sb_r, float* z0_out, float* x_out, int B,
                     int C, int T, alcm_stream_t stream);
/* alcm_wave_paste: blend a decoded region into the original waveform of a batch around the regenerated latent frames,
 * one launch (no reference counterpart: the reference has no edit path).
 *   orig, out (B, N); gen (B, Ng) holds samples gen_start .. gen_start + Ng of each clip; mask (B, T) per latent frame
 *   of frame_samples samples, a frame of mask > 0 is regenerated; ramp (R entries, device): the fade weights.
 *   d = distance in samples from sample n to the nearest sample of a regenerated frame of its clip (0 inside one, 1 on
 *   the first kept sample next to one); g = 1 at d = 0, ramp[d] for 0 < d < R, 0 from R on and outside gen;
 *   out = orig where g = 0 and gen where g = 1, both bit for bit, else orig + g * (gen - orig).
 * R = 0 (ramp may be NULL) is a hard switch at the frame edges.  out may be orig itself: then samples of g = 0 are
 * neither read nor written; any other overlap is not allowed.  The caller keeps ramp's reach inside gen (or accepts
 * the cut at gen's edges).  16-byte accesses when frame_samples, N, Ng and gen_start are multiples of 4 and orig, gen
 * and out are 16-byte aligned, element accesses otherwise.
 * ALCM_E_INVALID for a null orig, out or mask (gen with Ng > 0, ramp with R > 0), a negative size, frame_samples
 * outside 1 .. 2^20, T * frame_samples < N, gen_start + Ng > N, or R > 16 * frame_samples.  B, N or Ng of 0: no
 * launch (Ng = 0 out of place copies orig). */
int alcm_wave_paste(const float* orig, const float* gen, const float* mask, const float* ramp, float* out, int B,
                    int64_t N, int64_t gen_start, int64_t Ng, int T, int frame_samples, int R, alcm_stream_t stream);
/* alcm_wave_paste_ring: alcm_wave_paste on one period of a loop, one launch (the same kernel body; no reference
 * counterpart: the reference has no edit path).
 *   orig, out (B, N) with N = T * frame_samples exactly; mask (B, T) is circular; gen (B, Ng), 0 <= Ng <= N, holds the
 *   ring's samples (gen_start + i) mod N, i = 0 .. Ng - 1, 0 <= gen_start < N: it may go on across the wrap.
 *   d is measured round the ring: frame T - 1 is the left neighbour of frame 0, so a regenerated frame T - 1 fades into
 *   the first samples of frame 0 and a regenerated frame 0 into the last samples of frame T - 1.  g and out are
 *   alcm_wave_paste's: g = 1 at d = 0, ramp[d] for 0 < d < R, 0 from R on and outside gen; out = orig where g = 0 and
 *   gen where g = 1, both bit for bit, else the same fmaf(g, gen - orig, orig).
 * In place (out == orig) only the frames gen covers are visited, modulo T.  16-byte accesses under alcm_wave_paste's
 * conditions.
 * ALCM_E_INVALID for a null orig, out or mask (gen with Ng > 0, ramp with R > 0), a negative size, frame_samples
 * outside 1 .. 2^20, N != T * frame_samples, Ng > N, gen_start >= N, or R > 16 * frame_samples.  B, N or Ng of 0: no
 * launch (Ng = 0 out of place copies orig). */
int alcm_wave_paste_ring(const float* orig, const float* gen, const float* mask, const float* ramp, float* out, int B,
                         int64_t N, int64_t gen_start, int64_t Ng, int T, int frame_samples, int R,
                         alcm_stream_t stream);
/* alcm_seam_stats: the correlation and the level ratio of orig and gen where alcm_wave_paste_law is about to blend
 * them, two launches, nothing read back on the host (no reference counterpart).  orig, gen, mask, B, N, gen_start, Ng,
 * T, frame_samples and R are the paste's (alcm_wave_paste; ring != 0: alcm_wave_paste_ring's).
 *   A junction is a frame edge e (between the frames e - 1 and e, e = 0 .. T) of which exactly one is regenerated: an
 *   end of a maximal run of regenerated frames.  Frames outside 0 .. T - 1 count as kept on a line; on a ring frames and
 *   edges are taken modulo T, so edge T is edge 0.
 *   The zone of a junction: the samples of 0 < d < R that lie inside gen and whose d the paste measures from that
 *   junction.  A kept sample with dl samples to the last regenerated sample on its left and dr to the first on its
 *   right belongs to the left junction where dl < dr and to the right one otherwise (a tie goes right, as in the
 *   paste), so a kept gap shorter than 2 R is split exactly as the fade splits it.
 *   Per zone, in fp64 (the fp32 products are exact there), in a fixed order without atomics:
 *     Sxx = sum orig^2, Syy = sum gen^2, Sxy = sum orig * gen.
 *   rho = clamp(Sxy / (sqrt(Sxx) * sqrt(Syy)), 0, 1), and 1 where Sxx or Syy is zero (an empty or a silent zone) and
 *   at an edge that is no junction.
 *   gam of a run = clamp(sqrt((Sxx + Sxx') / (Syy + Syy')), 0.5, 2) over the run's two junctions (a run that touches
 *   the end of a line has an empty zone there; a run across the wrap of a ring is one run), and 1 where either pooled
 *   sum is zero or the run has no junction (a ring regenerated all round).
 * Outputs (device):
 *   rho  (B, T + 1) fp32, indexed by the edge; on a ring rho[b][T] = rho[b][0].
 *   gam  (B, T) fp32: the run's value in each of its frames, 1 in a kept frame.
 *   sums (B, T + 1, 3) fp64, 8-byte aligned: Sxx, Syy, Sxy per edge, zero at an edge that is no junction; on a ring
 *        entry T repeats entry 0.  gam is computed from these.
 * ALCM_E_INVALID under the paste's conditions in the paste's words (orig stands for out; no ramp is taken), and for a
 * null rho, gam or sums, or sums not 8-byte aligned.  B or T of 0: no launch. */
int alcm_seam_stats(const float* orig, const float* gen, const float* mask, int B, int64_t N, int64_t gen_start,
                    int64_t Ng, int T, int frame_samples, int R, int ring, float* rho, float* gam, double* sums,
                    alcm_stream_t stream);
/* alcm_wave_paste_law: alcm_wave_paste (ring != 0: alcm_wave_paste_ring) under a power-preserving fade law and a
 * per-run gain, one launch: the same tiling, mask search, g, in-place rule and conditions for 16-byte accesses.
 *   rho (B, T + 1) per frame edge and gam (B, T) per regenerated frame, as alcm_seam_stats writes them; rho NULL: 0
 *   everywhere (the equal-power law), gam NULL: 1.  A table of ones for rho gives the linear law up to rounding.
 *   y = gen where gam is NULL, else fl(gam * gen) with the gam of the sample's own frame at d = 0 and of the
 *   regenerated frame its d is measured from at d > 0 (dl < dr: the run on the left, else the one on the right); rho
 *   is the entry of the edge between that frame and the kept gap.
 *   out = orig where g = 0 (in place neither read nor written) and y where g = 1, both bit for bit; else, with every
 *   operation rounded to fp32 on its own, none contracted, in this order:
 *     a = 1 - g;  s = (a * orig) + (g * y);  p = ((a * a) + (g * g)) + (((a + a) * g) * rho);
 *     out = (1 / sqrt(p)) * s          (sqrt and the division correctly rounded)
 *   The 16-byte path and the element path run the same operations and give the same bits.  1 / sqrt(p) restores the
 *   power of two signals of equal power and correlation rho; with unequal powers it is the equal-sigma approximation,
 *   which gam makes good when it is used.
 * ALCM_E_INVALID as alcm_wave_paste (alcm_wave_paste_ring), under the name wave_paste_law. */
int alcm_wave_paste_law(const float* orig, const float* gen, const float* mask, const float* ramp, const float* rho,
                        const float* gam, float* out, int B, int64_t N, int64_t gen_start, int64_t Ng, int T,
                        int frame_samples, int R, int ring, alcm_stream_t stream);
/* alcm_resample: band-limited rational resampling of a batch of clips with the mean over the channels folded into
 * the read, one launch (no reference counterpart: the reference labels its 16 kHz samples with any rate it is given).
 *   x (B, N_in, channels), interleaved as a WAV file stores it; y (B, N_out), N_out = ceil(N_in * up / down);
 *   taps (up, ntaps), device: row r holds the filter at the offsets k + first - r / up, k = 0 .. ntaps - 1, in input
 *   samples (audiolcm_amd/resample.py plans it per rate pair: up / down = rate_out / rate_in in lowest terms);
 *   y[b][n] = sum_k taps[(n * down) mod up][k] * xm[b][floor(n * down / up) + first + k], xm the channel mean of x and 0
 *   outside [0, N_in): output n sits at input position n * down / up.
 * Index arithmetic is 64-bit.  Each output is one fp32 fmaf chain over k in rising order, whatever B, the output's
 * position or the alignment of x (element loads; 8-byte loads for stereo at an 8-byte aligned x).  No atomics.
 * ALCM_E_INVALID for a null x, y or taps, up, down or ntaps < 1, channels outside 1 .. 8, a negative size,
 * N_out != ceil(N_in * up / down), or a rate pair so far apart that 256 outputs' input window exceeds 48 KiB of LDS.
 * B or N_in of 0: no launch. */
int alcm_resample(const float* x, float* y, int B, int64_t N_in, int channels, int64_t N_out, int up, int down,
                  const float* taps, int ntaps, int first, alcm_stream_t stream);
/* alcm_loudness_hops: the K-weighted energy of a batch of mono clips per 100 ms hop and their sample peak (ITU-R
 * BS.1770; no reference counterpart: the reference writes the vocoder's waveform as it is).
 *   x (B, N) fp32, row stride ld >= N; y = x through the two biquads of coef in cascade from zero state;
 *   hop_sums_out[b][h] = sum of y^2 over the samples h * hop .. (h + 1) * hop, h = 0 .. N / hop - 1, (B, N / hop)
 *   fp64 (a trailing partial hop is left out); peak_out[b] = max |x[b][n]| (B) fp32, exact.
 *   coef (device, 154 fp64, audiolcm_amd/loudness.py tables(rate)): the high shelf's and the high pass's
 *   (b0, b1, b2, a1, a2), then the cascade's 4 x 4 state-transition matrix M (row-major, state s1, s2, t1, t2 of the
 *   transposed direct form II) to the powers 32 * 2^j, j = 0 .. 7, and 8192.
 * Either output may be NULL, not both; hop_sums_out NULL is a peak-only pass that does not read coef.  The
 * recursion runs in parallel over time: a thread per 32 samples, a workgroup per 8192, the states joined by a scan of
 * the chunks' affine maps; state and sums are fp64.  Three launches (two for peak only), no atomics: the partial sums
 * are added in rising order and a clip's bits depend on neither B, ld nor the other clips.  Index arithmetic is
 * 64-bit; 16-byte loads when x is 16-byte aligned and ld a multiple of 4, element loads otherwise, same values.
 * ws: alcm_loudness_workspace_bytes(B, N, hop) bytes of device memory, 8-byte aligned (0 for an empty or invalid
 * problem).  ALCM_E_INVALID for a null x, no output, hop_sums_out without coef, a negative B or N, hop < 1, ld < N or
 * a workspace that is null, misaligned or too small.  B or N of 0: no launch. */
size_t alcm_loudness_workspace_bytes(int B, int64_t N, int hop);
int alcm_loudness_hops(const float* x, int B, int64_t N, int64_t ld, const double* coef, int hop, double* hop_sums_out,
                       float* peak_out, void* ws, size_t ws_bytes, alcm_stream_t stream);
/* alcm_loudness_gain: gated integrated loudness of each clip from its hop sums, and the gain to a target under a peak
 * ceiling; one launch, one wave per clip, fp64, no host synchronisation.
 *   hop_sums (B, nh) fp64 and peak (B) fp32 as alcm_loudness_hops writes them; block j = hops j .. j + 3, nh - 3
 *   blocks: z_j = (S_j + S_j+1 + S_j+2 + S_j+3) / (4 hop), l_j = -0.691 + 10 log10 z_j;
 *   absolute gate: l_j > -70; relative gate: l_j > -0.691 + 10 log10(mean z of the blocks past the absolute gate) - 10;
 *   L = -0.691 + 10 log10(mean z of the blocks past both gates), -inf when none passes the absolute gate (or nh < 4);
 *   gain = 10^((target_lufs - L) / 20) rounded to fp32, 1 when target_lufs is NaN or L = -inf; then, with ceiling > 0
 *   (linear) and fl(peak * gain) > ceiling: gain = fl(ceiling / peak), stepped down one ulp while
 *   fl(peak * gain) > ceiling, so that no sample of |x| <= peak times gain exceeds the ceiling.
 * lufs_out, gain_out (B) fp32; either may be NULL, not both; peak may be NULL without a ceiling.
 * ALCM_E_INVALID for no output, a negative B or nh, hop < 1, null hop_sums with nh > 0 or a ceiling without peak.
 * B of 0: no launch. */
int alcm_loudness_gain(const double* hop_sums, const float* peak, int B, int64_t nh, int hop, float target_lufs,
                       float ceiling, float* lufs_out, float* gain_out, alcm_stream_t stream);
/* alcm_wave_gain: y[b][n] = x[b][n] * gain[b], one fp32 rounding; x (B, N) row stride ldx, y (B, N) row stride ldy,
 * gain (B) device.  y may be x itself; a gain of 1 leaves the bits as they are.  16-byte accesses when x and y are
 * 16-byte aligned and ldx, ldy multiples of 4, element accesses otherwise.
 * ALCM_E_INVALID for a null x, gain or y, a negative B or N, or a stride < N.  B or N of 0: no launch. */
int alcm_wave_gain(const float* x, const float* gain, float* y, int B, int64_t N, int64_t ldx, int64_t ldy,
                   alcm_stream_t stream);
/* alcm_limiter: a look-ahead peak limiter over a batch of mono clips (no reference counterpart), from the pre-gain
 * gain[b] (device), the linear ceiling c, the look-ahead La = lookahead samples and the release coefficient
 * a = release_coef = exp(-1 / (release_s * rate)).  Per clip, on x[0 .. N):
 *   1. u[n] = fl32(x[n] * gain), the rounding of alcm_wave_gain;
 *   2. e[n] = |u[n]|; with env (B, N * os) fp32, row stride ld_env, an oversampled copy of the clip, os 1 or 4:
 *      e[n] = max(|u[n]|, max over k < os of |fl32(env[n * os + k] * gain)|);
 *   3. r[n] = c / e[n] where e[n] > c, else 1; r = 1 outside [0, N);
 *   4. the hold: m[j] = min r[j .. j + La], j = -La .. N - 1;
 *   5. the attack: s[n] = mean m[n - La .. n]: every m of that window covers r[n], so s[n] <= r[n], and the gain
 *      reaches what a peak needs exactly at the peak after a linear ramp of La samples;
 *   6. the release: y[n] = min(s[n], a y[n-1] + (1 - a) s[n]), y[-1] = 1;
 *   7. out[n] = copysign(min(|fl32(u[n] * fl32(y[n]))|, c), u[n]): no |out| exceeds c whatever the rounding.
 * Steps 3 to 6 are fp64.  Two launches, no atomics, no host synchronisation.  A thread per 8 samples, a workgroup per
 * 2048 with La samples of halo either side in LDS: the hold is a sliding maximum of e by doubling (c / e is
 * monotone), the attack a prefix sum over the tile, and the release, whose steps y -> min(C, A y + D) are closed
 * under composition, a scan of three doubles per chunk in the workgroup and a fold of the workgroups' maps in rising
 * order.  s goes through ws, so the second launch reads only the samples it writes: y may be x itself and gives the
 * bits of the out-of-place call.  A clip's bits depend on neither B, the strides nor the other clips; a clip none of
 * whose e exceeds c gets alcm_wave_gain's bits.  Index arithmetic is 64-bit; 16-byte accesses to x (and y) when the
 * pointers are 16-byte aligned and the strides multiples of 4, to env with os = 4 likewise; element accesses
 * otherwise, same values.  env may be NULL: it is not read and os is ignored.
 * ws: alcm_limiter_workspace_bytes(B, N, lookahead) bytes of device memory, 8-byte aligned (0 for an empty or
 * invalid problem).  ALCM_E_INVALID, before any HIP call, for a null x, gain or y, os not 1 or 4 with an env, a
 * negative B or N, ldx or ldy < N, ld_env < N * os, a ceiling that is not finite and positive, lookahead outside
 * 0 .. 1024 (5 ms at 192 kHz), release_coef outside [0, 1), or a workspace that is null, misaligned or too small.
 * B or N of 0: no launch. */
size_t alcm_limiter_workspace_bytes(int B, int64_t N, int lookahead);
int alcm_limiter(const float* x, const float* env, int os, const float* gain, float* y, int B, int64_t N, int64_t ldx,
                 int64_t ld_env, int64_t ldy, float ceiling, int lookahead, double release_coef, void* ws,
                 size_t ws_bytes, alcm_stream_t stream);
/* out[b] = [f(v[b]*vscale*freqs[i]) ...]: cos_first ? [cos | sin] (TimestepEmbedder, concatDiT.py:49-67)
 *                                                   : [sin | cos] (get_guidance_scale_embedding, w*1000).
 * freqs: the reference's fp32 frequency table (half entries, device pointer) */
int alcm_sincos_embedding(const float* v, float vscale, const float* freqs, int B, int half, int cos_first,
                          float* out, alcm_stream_t stream);

/* ---------------------------------------------------------------- models
 * Weights are host fp32 tensors named by the reference state_dict keys. */
typedef struct alcm_named_tensor {
  const char* name;
  const float* data; /* HOST pointer, contiguous fp32 */
  int ndim;
  int64_t shape[4];
} alcm_named_tensor;

typedef struct alcm_model alcm_model;

/* kind: 0 = ConcatDiT2MLP, 1 = AutoencoderKL (decoder; + Encoder1D when encoder.* tensors are given), 2 = BigVGAN,
 * 3 = FrozenCLAPFLANEmbedder text encoders, 4 = log-mel front-end (NAT_mel.MelNet).
 * iconfig/fconfig: see DESIGN.md §C-ABI (hyper-parameters from configs/audiolcm.yaml / bigvgan json) */
enum { ALCM_MODEL_DIT = 0, ALCM_MODEL_VAE = 1, ALCM_MODEL_BIGVGAN = 2, ALCM_MODEL_TEXT = 3, ALCM_MODEL_MEL = 4 };
/* policy: ALCM_POLICY_* (below) */
int alcm_model_create(int kind, const int* iconfig, int n_iconfig, const alcm_named_tensor* tensors,
                      int n_tensors, int policy, alcm_model** out);
int alcm_model_destroy(alcm_model* m);
size_t alcm_model_weight_bytes(const alcm_model* m);
int alcm_model_set_split(alcm_model* m, int split);
/* per-layer precision policy: ALCM_POLICY_BF16 every contraction bf16; ALCM_POLICY_SPLIT every contraction
 * bf16x3 (fp32 parity); ALCM_POLICY_MIXED fp16 single MFMA on the layers the parity budget allows
 * (DiT GEGLU FFN convs, VAE k3 ResnetBlock/upsample convs, BigVGAN stage 0-2 AMPBlock convs: DESIGN.md §3),
 * bf16x3 elsewhere.  alcm_model_set_split(m, s) == set_precision(m, s ? SPLIT : BF16). */
enum { ALCM_POLICY_BF16 = 0, ALCM_POLICY_SPLIT = 1, ALCM_POLICY_MIXED = 2 };
int alcm_model_set_precision(alcm_model* m, int policy);
/* BigVGAN: run the three resblock chains of a stage concurrently on auxiliary streams forked from the caller's
 * stream (1, the default unless ALCM_SERIAL_RESBLOCKS is set at load) or serially on the caller's stream (0:
 * per-kernel timing, bench.py's roofline pass) */
int alcm_model_set_resblock_streams(alcm_model* m, int concurrent);
/* re-read the ALCM_* diagnostic environment switches (they are read once at library load) */
int alcm_reload_knobs(void);
/* diagnostics: what alcm_opconv (form == 0, n == 1), alcm_opconv_sum (form == 1, 1 <= n <= 3 terms) or
 * alcm_opconv_dense (form == 2, n == 1) would launch for these arguments under the current ALCM_* switches on a
 * device of ncu compute units (ncu <= 0: the current device's): one alcm_conv_plan_info per launch into out (room for
 * 3) and the launch count, or the ALCM_E* code the call itself would return (message in alcm_last_error()).  Host
 * only: pointers are tested for null-ness and alignment, never dereferenced, nothing is launched, and with ncu > 0 no
 * device is needed.
 * kernel: 0 lin_plane, 1 wconv3, 2 wconv3 sum form, 3 wconv2, 4 nconv, 5 opconv_kernel, 6 tconv_kernel (tail conv,
 * resident weights), 7 tconv2_kernel (tail conv, streamed weights); name: the profile row. */
typedef struct alcm_conv_plan_info {
  char name[160];
  int kernel, bm, bn;
  int64_t grid; /* workgroups of the conv launch */
  int ksplit;   /* K parts (1 = none; > 1 adds the reduction launch) */
  int n_major;
  int ncu;
  /* the tail convs only (empty / 0 elsewhere): the template-id of the instantiation but for its diagnostics flag,
   * which the profile row does not spell; threads per workgroup; column groups; 16-byte slots of an LDS weight row */
  char inst[96];
  int block, ncg, wslots;
  int tiles_per_batch; /* row tiles of one clip */
  int64_t tiles;       /* output tiles */
  double flops, bytes; /* the cost the profile row is charged */
} alcm_conv_plan_info;
int alcm_debug_conv_plan(const alcm_opconv_args* args, int n, int form, int ncu, alcm_conv_plan_info* out,
                         int* launches);
/* diagnostics: what alcm_gemm would launch for these arguments under the current ALCM_* switches (alcm_gemmplan.h), or
 * the ALCM_E* code the call itself would return (message in alcm_last_error()).  Host only: pointers are tested for
 * null-ness and alignment, never dereferenced, nothing is launched and no device is needed.
 * family: 0 nothing (M or N <= 0), 1 conv_kernel (window conv), 2 gemm_skinny_kernel, 3 gemm_kernel; name: the profile
 * row; bm, bn, wm, wn: tile and wave grid (skinny: rows / columns per workgroup); grid: workgroups in x, y, z. */
typedef struct alcm_gemm_plan_info {
  char name[128];
  int family;
  int bm, bn, wm, wn;
  int grid[3];
  double flops, bytes; /* the cost the profile row is charged */
} alcm_gemm_plan_info;
int alcm_debug_gemm_plan(const alcm_gemm_args* args, alcm_gemm_plan_info* out);
/* diagnostics: what alcm_activation1d_planes (and with it alcm_activation1d_op / _f16in) would launch for these
 * arguments under the current ALCM_* switches (alcm_actplan.h), or the ALCM_E* code the call itself would return.  Host
 * only, as alcm_debug_gemm_plan.
 * kernel: 0 act_coop_kernel<prec, np, nset>, 1 act_mfma_kernel<64, defer, in16>, 2 act_mfma3_kernel<64>; name: the
 * profile row; grid: workgroups of 256 threads; tiles_t, tiles_c, strips_t, y_lo: the kernel's scalar arguments (0
 * where the kernel has none). */
typedef struct alcm_act_plan_info {
  char name[64];
  int kernel;
  int prec, np, nset, defer, in16;
  int64_t grid;
  int tiles_t, tiles_c, strips_t;
  int64_t y_lo;
  double flops, bytes; /* the cost the profile row is charged */
} alcm_act_plan_info;
int alcm_debug_act_plan(const alcm_act_args* args, alcm_act_plan_info* out);
/* diagnostics: the same for alcm_flash_attention_ex (alcm_attnplan.h).  form: 0 flash_attn_res_kernel<prec, bias, true>
 * on operand rows, 1 flash_attn_res_kernel<prec, bias, false> on fp32 rows, 2 flash_attn_kernel<prec>; lp: keys padded
 * to the key tile; scale: the resolved score scale; grid, block: workgroups and threads of each. */
typedef struct alcm_attn_plan_info {
  char name[80];
  int form;
  int prec, bias;
  int lp, dh;
  float scale;
  int64_t grid;
  int block;
  double flops, bytes;
} alcm_attn_plan_info;
int alcm_debug_attn_plan(const alcm_attn_args* args, alcm_attn_plan_info* out);
/* The BigVGAN stage planner (alcm_vocplan.h).  A stage's static shape: the upsampler ConvTranspose1d cin -> cout
 * at `rate` as `rate` phase convs of `taps` taps on input rows padded to `cpad` channels, and nrb AMPBlock1 resblocks of
 * kernel size rb_k[j] with the ndil dilations dil[] (one set for the stage's resblocks). */
enum { ALCM_VOC_MAX_RB = 8, ALCM_VOC_MAX_DIL = 8 };
typedef struct alcm_voc_stage_shape {
  int cin, cout, rate, taps, cpad;
  int phases_share;  /* the phases' packed weights share kpad and the lo-plane offset */
  int dense_weights; /* the resblock convs also have the tail convs' dense packing */
  int act0_equal;    /* the resblocks' first Activation1d FIR taps are equal */
  int nrb, rb_k[ALCM_VOC_MAX_RB];
  int ndil, dil[ALCM_VOC_MAX_DIL];
} alcm_voc_stage_shape;
/* What a stage runs.  ups: 0 = phase convs on operand planes of the stage input, 1 = both phases of a
 * stride-2 stage in one split-precision pass (ups2), 2 = fp32-operand phase convs.  amp: 0 = fused (Activation1d in
 * the conv epilogues), 1 = fused on the tail convs' dense weights, 2 = wide (standalone Activation1d). */
typedef struct alcm_voc_stage_plan {
  int prec;             /* ALCM_PREC_* of the AMPBlock convs (and of a planes-form upsampler) */
  int ups;
  int planes_from_prev; /* ups == 0: the previous stage's sum-form close wrote the input planes */
  int amp;
  int h16;              /* wide: conv1 hands its Activation1d an fp16 plane */
  int act3;             /* the three chains' first Activation1d in one launch */
  int concurrent;       /* chains 1.. on the auxiliary streams */
  int own_bufs;         /* chain j works in its own buffers (otherwise every chain in chain 0's) */
  int sum3;             /* wide: the three chains' last conv2 + residual as one alcm_opconv_sum call */
  int writes_next;      /* sum3: one launch, which writes the next stage's input planes instead of fp32 */
} alcm_voc_stage_plan;
/* diagnostics: the plans alcm_bigvgan_forward would execute for n stages at batch B and M mel frames under `policy`
 * (ALCM_POLICY_*) and the current ALCM_* switches, with the resblock streams on or off, on ncu compute units (<= 0:
 * the current device's), one per stage into out.  Host only; with ncu > 0 no device is needed. */
int alcm_debug_voc_plan(const alcm_voc_stage_shape* shapes, int n, int policy, int streams, int B, int M, int ncu,
                        alcm_voc_stage_plan* out);
/* diagnostics: the K-part count both K-split users take (alcm_convplan.h ksplit_parts) */
int alcm_debug_ksplit_parts(int64_t tiles, int64_t slots, int chunks, double elems, double ws_floats);
/* diagnostics: the BigVGAN tail-conv phase trace (ALCM_TCONV_TRACE=1, which selects the tail convs' diagnostics
 * instantiations): shader-clock cycles summed over waves and tiles for [window + first slices, K loop, post-loop
 * barrier, staging, residual + state, Activation1d, final barrier] and the wave-tile count, since the last reset;
 * reset != 0 zeroes it.  The first call allocates the trace buffer and returns zeros (launches after it are traced).
 * Synchronizes the device.  ALCM_E_INVALID for a null out8. */
int alcm_debug_tconv_trace(unsigned long long* out8, int reset);
/* diagnostics: workgroup residency records of the last traced resident-weight tail conv (ALCM_TCONV_TRACE=1): per
 * workgroup [entry s_memrealtime, exit s_memrealtime, HW_ID, XCC_ID] into out (4 x n_wg values, at most 2048
 * workgroups); returns the count copied (0 before the first alcm_debug_tconv_trace call).  Synchronizes the device. */
int alcm_debug_tconv_wg_times(unsigned long long* out, int n_wg);

/* ---------------------------------------------------------------- model entry points and their workspaces
 * Every model entry point below takes a caller workspace `ws` of `ws_bytes` bytes of device memory, 256-byte aligned;
 * the alcm_*_workspace_bytes query next to it gives the size for the handle's precision policy and the shape
 * (alcm_dit_embed_context: alcm_dit_workspace_bytes(m, B, 1) is enough).  A smaller or null workspace is refused
 * with ALCM_E_WORKSPACE before anything is launched or written.  The workspace contract, for all of them:
 *   - contents on entry are irrelevant: the result does not depend on what [ws, ws + ws_bytes) holds, so one arena may
 *     serve calls of any shapes, policies and models, one after the other on a stream, without being cleared;
 *   - nothing outside [ws, ws + ws_bytes) is written, apart from the output tensor (the inputs are only read);
 *   - contents on exit are unspecified.
 * (tests/test_gpu_workspace.py: guarded workspaces of exactly the queried size, filled with NaN patterns.) */

/* DiT.  x (B,C_lat,T) NCT, t (B,) int64, ctx (B,154,1024), w_emb (B,256) -> eps (B,C_lat,T) NCT.
 * cemb_cache: (B,154,hidden) device buffer filled by alcm_dit_embed_context (step-invariant, hoisted). */
size_t alcm_dit_workspace_bytes(const alcm_model* m, int B, int T);
int alcm_dit_embed_context(alcm_model* m, const float* ctx, int B, float* cemb_cache, void* ws,
                           size_t ws_bytes, alcm_stream_t stream);
int alcm_dit_forward(alcm_model* m, const float* x, const int64_t* t, const float* cemb_cache,
                     const float* w_emb, float* eps_out, int B, int T, void* ws, size_t ws_bytes,
                     alcm_stream_t stream);

/* VAE decode_first_stage. z (B,20,T) NCT -> mel (B,80,2T) NCT */
size_t alcm_vae_workspace_bytes(const alcm_model* m, int B, int T);
int alcm_vae_decode(alcm_model* m, const float* z, float inv_scale_factor, float* mel_out, int B, int T,
                    void* ws, size_t ws_bytes, alcm_stream_t stream);

/* VAE encode_first_stage (AutoencoderKL.encode, autoencoder1d.py:54-58 -> Encoder1D :319-413 + quant_conv):
 * mel (B,80,M) NCT -> posterior moments (B, 2*embed_dim, To) NCT = [mean | logvar] before the clamp,
 * To = alcm_vae_encode_len(m, M) (M/2 for audiolcm.yaml).  Needs a model created with encoder.* tensors. */
size_t alcm_vae_encode_workspace_bytes(const alcm_model* m, int B, int M);
int alcm_vae_encode(alcm_model* m, const float* mel, float* moments_out, int B, int M, void* ws, size_t ws_bytes,
                    alcm_stream_t stream);
int alcm_vae_encode_len(const alcm_model* m, int M);

/* Log-mel front-end (ldm/data/preprocess/NAT_mel.py:66-85, MelNet.forward with center=False): wav (B, L) fp32,
 * L % hop == 0 -> mel (B, n_mels, L/hop) NCT = log10(clamp(mel_basis @ |STFT(reflect_pad(clamp(wav)))|, 1e-5)).
 * Model kind ALCM_MODEL_MEL, iconfig {n_fft, hop, win, n_mels}, tensors "window" (win) and "mel_basis"
 * (n_mels, n_fft/2+1). */
size_t alcm_mel_workspace_bytes(const alcm_model* m, int B, int L);
int alcm_mel_spectrogram(alcm_model* m, const float* wav, float* mel_out, int B, int L, void* ws, size_t ws_bytes,
                         alcm_stream_t stream);

/* BigVGAN. mel (B,80,M) NCT -> wav (B,1,256*M) */
size_t alcm_bigvgan_workspace_bytes(const alcm_model* m, int B, int M);
int alcm_bigvgan_forward(alcm_model* m, const float* mel, float* wav_out, int B, int M, void* ws,
                         size_t ws_bytes, alcm_stream_t stream);

/* Text conditioning: FrozenCLAPFLANEmbedder.encode (ldm/modules/encoders/modules.py:567-582) from token ids.
 * clap_ids / t5_ids (B, L) int64 DEVICE (the CLAP-BERT and T5 tokenizers' input_ids, L <= max_len = 77,
 * ids in [0, vocab): out-of-range ids embed as zero rows) -> out (B, 2L, 1024) fp32 DEVICE =
 * [Projection(BERT(clap_ids)) | T5Encoder(t5_ids)], no attention mask (as the reference).
 * iconfig (14 ints): bert vocab, hidden, layers, heads, intermediate, max_position, projection out,
 * t5 vocab, d_model, d_kv, heads, d_ff, layers, max_len.  Tensors: caption_encoder.base.* (BertModel),
 * caption_encoder.projection.*, t5_transformer.* (T5EncoderModel) plus "_alcm.t5_rel_buckets" (max_len x
 * max_len, the bidirectional relative-position bucket of j - i as float). */
size_t alcm_text_workspace_bytes(const alcm_model* m, int B, int L);
int alcm_text_encode(alcm_model* m, const int64_t* clap_ids, const int64_t* t5_ids, float* out, int B, int L,
                     void* ws, size_t ws_bytes, alcm_stream_t stream);

/* ---------------------------------------------------------------- live kernel timing (bench.py roofline)
 * Between begin/end every kernel launch is bracketed by hipEvents on its stream; end synchronises
 * and returns per-kernel aggregates keyed by the demangled kernel name rocprofv3 reports.
 * flops/bytes are ALGORITHMIC (2*M*N*K for GEMMs; unique input + weight + output bytes). */
typedef struct alcm_prof_entry {
  char name[128];
  int64_t launches;
  double total_ms;
  double flops;
  double bytes;
  double roof_ms; /* sum over launches of max(flops/peak_flops, bytes/peak_bw) */
  /* the HBM-bound launches of this entry (algorithmic flops/bytes below peak_flops/peak_bw) */
  int64_t hbm_launches;
  double hbm_ms;
  double hbm_bytes;
} alcm_prof_entry;
int alcm_profile_begin(double peak_flops, double peak_bytes_per_s);
int alcm_profile_end(alcm_prof_entry* out, int max_entries, int* n_entries);

#ifdef __cplusplus
}
#endif
#endif /* AUDIOLCM_HIP_H */
