// Internal (non-ABI) declarations shared by the libaudiolcm_hip.so translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "audiolcm_hip.h"
#include "alcm_actplan.h"
#include "alcm_attnplan.h"
#include "alcm_convplan.h"
#include "alcm_knobs.h"
#include "alcm_vocplan.h"

namespace alcm {

int set_error(int code, const std::string& msg);

#define ALCM_HIP(expr)                                                                         \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return ::alcm::set_error(ALCM_E_HIP, std::string(#expr ": ") + hipGetErrorString(_e));   \
  } while (0)

#define ALCM_TRY(expr)      \
  do {                      \
    int _r = (expr);        \
    if (_r) return _r;      \
  } while (0)

int gemm(const alcm_gemm_args& g, hipStream_t s);
int pack_conv_weight(const float* w, int c_out, int c_in, int k, int cpad, int kpad, int transposed, int stride,
                     int phase, void* out, hipStream_t s);

int group_norm_affine(const float* x, int B, int T, int C, int64_t sb, int64_t st, int groups, float eps,
                      const float* gamma, const float* beta, float* scale, float* shift, hipStream_t s);
int row_stats(const float* x, int rows, int C, int64_t ld, float eps, float* mean, float* rstd, hipStream_t s);
int layer_norm(const float* x, int rows, int C, int64_t ld_in, float eps, const float* gamma, const float* beta,
               const float* add, int64_t ld_add, float* y, int64_t ld_out, hipStream_t s, int rpb = 0,
               int64_t out_bs = 0);
int softmax_rows(float* x, int rows, int n, int64_t ld, hipStream_t s);
int layer_norm_plane(const float* x, int rows, int C, int64_t ld, float eps, const float* gamma, const float* beta,
                     void* plane, int prec, hipStream_t s);
// plane[b][t'][c] = (silu?)(x[b][t'/up][c] * scale[b][c] + shift[b][c]) (scale == nullptr: identity)
int affine_plane(const float* x, int B, int T, int C, int up, const float* scale, const float* shift, int silu,
                 void* plane, int prec, hipStream_t s);
int activation1d(const float* x, float* y, int B, int T, int C, int64_t sb, int64_t st, const float* alpha_exp,
                 const float* inv_beta, const float* up_filter, const float* down_filter, hipStream_t s);
int lcm_step(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise,
             const float* coeffs, float* prev, float* den, int64_t n, hipStream_t s);
int lcm_step_edit(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise,
                  const float* coeffs, const float* z0, const float* mask, float* prev, float* den, int B, int C, int T,
                  hipStream_t s);
int lcm_step_joint(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise,
                   const float* coeffs, const int* starts, int K, const float* wn, float* prev, float* den, float* xw,
                   int B, int C, int L, int W, hipStream_t s);
int lcm_step_joint_edit(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise,
                        const float* coeffs, const int* starts, int K, const float* wn, const float* z0,
                        const float* mask, float* prev, float* den, float* xw, int B, int C, int L, int W,
                        hipStream_t s);
int lcm_step_ring(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise,
                  const float* coeffs, const int* starts, int K, const float* wn, float* prev, float* den, float* xw,
                  int B, int C, int L, int W, hipStream_t s);
int lcm_step_ring_edit(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise,
                       const float* coeffs, const int* starts, int K, const float* wn, const float* z0,
                       const float* mask, float* prev, float* den, float* xw, int B, int C, int L, int W,
                       hipStream_t s);
int wave_loop(const float* ext, const float* ramp, float* out, int B, int64_t Next, int64_t start, int64_t N, int R,
              hipStream_t s);
int latent_init(const float* moments, const float* z0_in, const float* e0, float scale, const float* noise,
                const float* mask, float sa, float sb, float sa_r, float sb_r, float* z0_out, float* x_out, int B,
                int C, int T, hipStream_t s);
int wave_paste(const float* orig, const float* gen, const float* mask, const float* ramp, float* out, int B, int64_t N,
               int64_t gen_start, int64_t Ng, int T, int fs, int R, hipStream_t s);
int wave_paste_ring(const float* orig, const float* gen, const float* mask, const float* ramp, float* out, int B,
                    int64_t N, int64_t gen_start, int64_t Ng, int T, int fs, int R, hipStream_t s);
int wave_paste_law(const float* orig, const float* gen, const float* mask, const float* ramp, const float* rho,
                   const float* gam, float* out, int B, int64_t N, int64_t gen_start, int64_t Ng, int T, int fs, int R,
                   int ring, hipStream_t s);
int seam_stats(const float* orig, const float* gen, const float* mask, int B, int64_t N, int64_t gen_start, int64_t Ng,
               int T, int fs, int R, int ring, float* rho, float* gam, double* sums, hipStream_t s);
int fill_f32(float* p, int64_t n, float v, hipStream_t s);
int nct_to_cl(const float* x, int B, int C, int T, int Cp, float* y, hipStream_t s);
// fp32 rows [rows][C] -> operand planes [rows][Cp] in the format of `prec` (SPLIT: lo plane rows * Cp after hi)
int to_planes(const float* x, void* y, int64_t rows, int C, int Cp, int prec, hipStream_t s);
// BigVGAN output head: Activation1d -> conv_post (k7, C -> 1, weights [tap][C] fp32) -> tanh, fp32 (alcm_act.hip)
struct Taps12O;
int act_conv_post(const float* x, float* wav, int B, int T, int C, const float* alpha_exp, const float* inv_beta,
                  const Taps12O& f, const float* w_tc, float bias, hipStream_t s);
// Activation1d into MFMA operand planes (alcm_act.hip): planned by act_plan (alcm_actplan.h), which holds every check
// and the choice between the VALU kernel and the MFMA-FIR kernels; activation1d_planes only launches.  The three
// below are its argument forms: three parameter sets of one input, one set, one set of an fp16 plane x16 [B][T][C]
// (the wide-stage conv1 output, alcm_opconv's out_plane; the MFMA kernel's shapes only, ALCM_E_INVALID otherwise)
int activation1d_planes(const alcm_act_args& a, hipStream_t s);
int activation1d_x3(const float* x, void* const y[3], int B, int T, int C, int Cp, const float* const alpha_exp[3],
                    const float* const inv_beta[3], const float* up_filter, const float* down_filter, int prec,
                    hipStream_t s);
int activation1d_op(const float* x, void* y, int B, int T, int C, int Cp, const float* alpha_exp,
                    const float* inv_beta, const float* up_filter, const float* down_filter, int prec,
                    hipStream_t s);
int activation1d_op_h16(const void* x16, void* y, int B, int T, int C, int Cp, const float* alpha_exp,
                        const float* inv_beta, const float* up_filter, const float* down_filter, int prec,
                        hipStream_t s);
int opconv(const alcm_opconv_args& a, hipStream_t s);
// The fused attention (alcm_attn.hip): planned by attn_plan (alcm_attnplan.h), the launcher switches once on the plan.
// o_plane != nullptr: write the output as an fp16 / bf16 operand plane [B][L][H] instead of fp32 O
// bias != nullptr: + bias[(head * bld + query) * bld + key] on the scores (L <= 512); scale > 0 replaces 1/sqrt(dh);
// qkv_plane != nullptr (then qkv == nullptr): q / k / v rows as PREC operand elements (L <= 512)
int flash_attention(const float* qkv, float* O, int B, int L, int H, int nh, int prec, hipStream_t s,
                    void* o_plane = nullptr, const float* bias = nullptr, int bld = 0, float scale = 0.f,
                    const void* qkv_plane = nullptr);
int opconv_sum(const alcm_opconv_args* a, int n, hipStream_t s);
// the launches of a ConvPlan (alcm_convplan.h), one per kernel file: fill the kernel's argument struct, pick the
// instantiation the plan names, launch, record the profile row
int lin_plane_launch(const ConvPlan& pl, const alcm_opconv_args& a, hipStream_t s);                    // alcm_sgemm.hip
int wconv_launch(const ConvPlan& pl, const alcm_opconv_args& a, hipStream_t s);                        // alcm_wconv.hip
int wconv3_sum_launch(const ConvPlan& pl, const alcm_opconv_args* a, int n, hipStream_t s);            // alcm_wconv.hip
int nconv_launch(const ConvPlan& pl, const alcm_opconv_args& a, hipStream_t s);                        // alcm_nconv.hip

// alcm_opconv_dense: the narrow AMPBlock conv on dense weights (a.w / w_lo_off / kpad as the C entry defines them),
// planned by dense_conv_plan and launched by alcm_tconv.hip
int opconv_dense(const alcm_opconv_args& a, hipStream_t s);

struct Taps12O;

// BigVGAN stride-2 / kernel-4 upsampler, both phases in one split-precision pass (alcm_ups.hip; where ups2_supported,
// alcm_vocplan.h)
int ups2(const float* x, float* out, int B, int T, int cin, int cout, const unsigned short* w0, const unsigned short* w1,
         int64_t lo, int kpad, const int pad[2], const int off[2], const float* bias, hipStream_t s);
// bf16x3 1x1 conv on split operand planes (alcm_sgemm.hip)
bool sgemm_planes_ok(int K, int N, int kpad);
int sgemm_planes(const unsigned short* a, int64_t a_lo, int M, int K, const unsigned short* w, int64_t w_lo, int kpad,
                 int N, const float* bias, const float* res, int64_t ldr, float* out, int64_t ldo, float out_scale,
                 hipStream_t s);
int split_planes(const float* x, int64_t rows, int C, int T, const float* scale, const float* shift,
                 unsigned short* y, hipStream_t s);

// compute units of the current device, queried once (256 where the query fails or answers fewer than 8)
inline int device_cus() {
  static const int ncu = [] {
    int dev = 0, n = 0;
    return (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n >= 8)
               ? n
               : 256;
  }();
  return ncu;
}

bool prof_enabled();
void* prof_start(hipStream_t s);
void prof_stop(void* tok, hipStream_t s, const std::string& name, double flops, double bytes);

constexpr int kBK = 32;
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

}  // namespace alcm
