// Bandwidth-bound kernels of the AudioLCM hot path (gfx950): norm statistics, softmax,
// the fused anti-aliased SnakeBeta activation (Activation1d), the LCM step and the
// sinusoidal embeddings.  All tensors are fp32; activations are channels-last (b, t, c).
#include <algorithm>
#include <vector>

#include "alcm_common.h"
#include "alcm_internal.h"

namespace alcm {

// ---------------------------------------------------------------- block reduction helpers
template <typename T>
__device__ __forceinline__ T wave_sum_t(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T>
__device__ T block_sum(T v, T* sh) {  // blockDim.x == 256
  v = wave_sum_t(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sh[w] = v;
  __syncthreads();
  T r = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return r;
}

// ---------------------------------------------------------------- GroupNorm -> per-(b,c) affine
// torch.nn.GroupNorm (Normalize, new_attention.py:85-86 / autoencoder1d.py:168-169, and the
// DiT final GN16): biased variance over (C/G channels x T), y = (x-mean)*rstd*gamma + beta.
// Emitted as scale = rstd*gamma, shift = beta - mean*scale, consumed by the next GEMM's prologue.
__global__ __launch_bounds__(256) void gn_affine_kernel(const float* __restrict__ x, int T, int C, int64_t sb,
                                                        int64_t st, int groups, float eps,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* scale, float* shift,
                                                        FastDiv cgdiv) {
  __shared__ double sh[4];
  const int g = blockIdx.x, b = blockIdx.y;
  const int cg = C / groups;
  const float* base = x + (int64_t)b * sb + g * cg;
  const int64_t n = (int64_t)cg * T;
  // one pass over the group: fp64 sum and sum of squares (53-bit accumulation of fp32 inputs, so
  // E[x^2] - mean^2 keeps fp32-level accuracy for any mean/std ratio these activations reach)
  double s = 0.0, q = 0.0;
  for (int64_t e = threadIdx.x; e < n; e += 256) {
    uint32_t t, c;
    cgdiv.divmod((uint32_t)e, t, c);
    const double x1 = (double)base[(int64_t)t * st + c];
    s += x1;
    q += x1 * x1;
  }
  const double mean = block_sum(s, sh) / (double)n;
  const double var = fmax(block_sum(q, sh) / (double)n - mean * mean, 0.0);
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const float fmean = (float)mean;
  for (int c = threadIdx.x; c < cg; c += 256) {
    const int ch = g * cg + c;
    const float sc = rstd * gamma[ch];
    scale[(int64_t)b * C + ch] = sc;
    shift[(int64_t)b * C + ch] = beta[ch] - fmean * sc;
  }
}

// the same statistics read as float4 pieces (C / groups % 4 == 0, 16-B aligned rows): a quarter of the load
// instructions and index divisions; the fp64 sums see the same values in another order (53-bit accumulation of the
// fp32 inputs: the fp32 mean / rstd it rounds to are unaffected in practice)
__global__ __launch_bounds__(256) void gn_affine4_kernel(const float* __restrict__ x, int T, int C, int64_t sb,
                                                         int64_t st, int groups, float eps,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* scale, float* shift,
                                                         FastDiv cg4div) {
  __shared__ double sh[4];
  const int g = blockIdx.x, b = blockIdx.y;
  const int cg = C / groups;
  const float* base = x + (int64_t)b * sb + g * cg;
  const int64_t n4 = (int64_t)(cg / 4) * T;
  double s = 0.0, q = 0.0;
  for (int64_t e = threadIdx.x; e < n4; e += 256) {
    uint32_t t, c4;
    cg4div.divmod((uint32_t)e, t, c4);
    const float4 v = *reinterpret_cast<const float4*>(base + (int64_t)t * st + 4 * c4);
    const double a0 = v.x, a1 = v.y, a2 = v.z, a3 = v.w;
    s += (a0 + a1) + (a2 + a3);
    q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
  }
  const double n = (double)cg * T;
  const double mean = block_sum(s, sh) / n;
  const double var = fmax(block_sum(q, sh) / n - mean * mean, 0.0);
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const float fmean = (float)mean;
  for (int c = threadIdx.x; c < cg; c += 256) {
    const int ch = g * cg + c;
    const float sc = rstd * gamma[ch];
    scale[(int64_t)b * C + ch] = sc;
    shift[(int64_t)b * C + ch] = beta[ch] - fmean * sc;
  }
}

int group_norm_affine(const float* x, int B, int T, int C, int64_t sb, int64_t st, int groups, float eps,
                      const float* gamma, const float* beta, float* scale, float* shift, hipStream_t s) {
  if (!x || !gamma || !beta || !scale || !shift || B <= 0 || T <= 0 || groups <= 0 || C % groups)
    return set_error(ALCM_E_INVALID, "group_norm_affine: bad arguments");
  const int cg = C / groups;
  if (cg % 4 == 0 && st % 4 == 0 && sb % 4 == 0 && !(((uintptr_t)x) & 15))
    hipLaunchKernelGGL(gn_affine4_kernel, dim3(groups, B), dim3(256), 0, s, x, T, C, sb, st, groups, eps, gamma, beta,
                       scale, shift, FastDiv((uint32_t)(cg / 4)));
  else
    hipLaunchKernelGGL(gn_affine_kernel, dim3(groups, B), dim3(256), 0, s, x, T, C, sb, st, groups, eps, gamma, beta,
                       scale, shift, FastDiv((uint32_t)cg));
  ALCM_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- LayerNorm (per-row statistics)
// nn.LayerNorm(576), eps 1e-5 (concatDiT.py:114-116, 97-99).  One wave per row, two-pass.
template <bool APPLY>
__global__ __launch_bounds__(256) void ln_kernel(const float* __restrict__ x, int rows, int C, int64_t ld, float eps,
                                                 float* mean_out, float* rstd_out, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, const float* __restrict__ add,
                                                 int64_t ld_add, float* y, int64_t ld_out, int rpb, int64_t out_bs) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (int64_t)row * ld;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  const float mean = wave_sum(s) / (float)C;
  float v = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = xr[c] - mean;
    v += d * d;
  }
  const float var = wave_sum(v) / (float)C;
  const float rstd = 1.0f / sqrtf(var + eps);
  if (!APPLY) {
    if (lane == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
    return;
  }
  // rpb > 0: rows come in batches of rpb; the add row is the row within its batch, output batch bb starts at row
  // bb * out_bs (the DiT condition tokens: one launch for every clip, written into the [B][CT] token rows)
  int64_t arow = row, orow = row;
  if (rpb > 0) {
    const int bb = row / rpb, t = row - bb * rpb;
    arow = t;
    orow = (int64_t)bb * out_bs + t;
  }
  float* yr = y + orow * ld_out;
  const float* ar = add ? add + arow * ld_add : nullptr;
  for (int c = lane; c < C; c += 64) {
    float o = (xr[c] - mean) * rstd * gamma[c] + beta[c];
    if (ar) o += ar[c];
    yr[c] = o;
  }
}

int row_stats(const float* x, int rows, int C, int64_t ld, float eps, float* mean, float* rstd, hipStream_t s) {
  if (!x || !mean || !rstd || rows <= 0 || C <= 0) return set_error(ALCM_E_INVALID, "row_stats: bad arguments");
  hipLaunchKernelGGL(ln_kernel<false>, dim3((rows + 3) / 4), dim3(256), 0, s, x, rows, C, ld, eps, mean, rstd,
                     nullptr, nullptr, nullptr, (int64_t)0, nullptr, (int64_t)0, 0, (int64_t)0);
  ALCM_HIP(hipGetLastError());
  return 0;
}

int layer_norm(const float* x, int rows, int C, int64_t ld_in, float eps, const float* gamma, const float* beta,
               const float* add, int64_t ld_add, float* y, int64_t ld_out, hipStream_t s, int rpb, int64_t out_bs) {
  if (!x || !y || !gamma || !beta || rows <= 0 || C <= 0 || rpb < 0) return set_error(ALCM_E_INVALID, "layer_norm: bad arguments");
  hipLaunchKernelGGL(ln_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, s, x, rows, C, ld_in, eps, nullptr, nullptr,
                     gamma, beta, add, ld_add, y, ld_out, rpb, out_bs);
  ALCM_HIP(hipGetLastError());
  return 0;
}

// LayerNorm straight into an MFMA operand plane (fp16 or bf16 [rows][C]) for a conv that reads planes
// (DiT Conv1dFeedForward input, concatDiT.py:120-125 / new_attention.py:48-74)
template <int PREC>
__global__ __launch_bounds__(256) void ln_plane_kernel(const float* __restrict__ x, int rows, int C, int64_t ld,
                                                       float eps, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, u16* __restrict__ y) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (int64_t)row * ld;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  const float mean = wave_sum(s) / (float)C;
  float v = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = xr[c] - mean;
    v += d * d;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)C + eps);
  u16* yr = y + (int64_t)row * C;
  for (int c = lane; c < C; c += 64) {
    const float o = (xr[c] - mean) * rstd * gamma[c] + beta[c];
    yr[c] = PREC == PREC_F16 ? __builtin_bit_cast(u16, (_Float16)o) : __builtin_bit_cast(u16, (__bf16)o);
  }
}

int layer_norm_plane(const float* x, int rows, int C, int64_t ld, float eps, const float* gamma, const float* beta,
                     void* plane, int prec, hipStream_t s) {
  if (!x || !plane || !gamma || !beta || rows <= 0 || C <= 0 || (prec != PREC_F16 && prec != PREC_BF16))
    return set_error(ALCM_E_INVALID, "layer_norm_plane: bad arguments");
  if (prec == PREC_F16)
    hipLaunchKernelGGL(ln_plane_kernel<PREC_F16>, dim3((rows + 3) / 4), dim3(256), 0, s, x, rows, C, ld, eps, gamma,
                       beta, (u16*)plane);
  else
    hipLaunchKernelGGL(ln_plane_kernel<PREC_BF16>, dim3((rows + 3) / 4), dim3(256), 0, s, x, rows, C, ld, eps, gamma,
                       beta, (u16*)plane);
  ALCM_HIP(hipGetLastError());
  return 0;
}

// GroupNorm affine (+ swish) straight into an MFMA operand plane, optionally nearest-upsampled along t:
// plane[b][t'][c] = act(x[b][t'/up][c] * scale[b][c] + shift[b][c]).  The VAE decoder's
// norm -> nonlinearity -> conv k3 (ResnetBlock1D, autoencoder1d.py:212-235) and Upsample1D's
// interpolate(nearest) -> conv (autoencoder1d.py:291-295) then run on the wide-layer conv kernel.
// One workgroup per output row, 4 channels per thread (C % 4 == 0, contiguous (B, T, C) input).
template <int PREC, bool SILU>
__global__ __launch_bounds__(256) void affine_plane_kernel(const float* __restrict__ x, int T, int C, int up,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift, u16* __restrict__ y) {
  const int row = blockIdx.x;  // b * (T * up) + t'
  const int To = T * up;
  const int b = row / To, to = row - b * To;
  const float4* xr = reinterpret_cast<const float4*>(x + ((int64_t)b * T + to / up) * C);
  const float4* sc = scale ? reinterpret_cast<const float4*>(scale + (int64_t)b * C) : nullptr;
  const float4* sh = scale ? reinterpret_cast<const float4*>(shift + (int64_t)b * C) : nullptr;
  uint2* yr = reinterpret_cast<uint2*>(y + (int64_t)row * C);
  auto cv = [](float o) -> uint32_t {
    if (SILU) o = o / (1.0f + __expf(-o));
    return PREC == PREC_F16 ? (uint32_t)__builtin_bit_cast(u16, (_Float16)o)
                            : (uint32_t)__builtin_bit_cast(u16, (__bf16)o);
  };
  for (int c = threadIdx.x; c < C / 4; c += 256) {
    float4 v = xr[c];
    if (sc) {
      const float4 a = sc[c], h = sh[c];
      v.x = v.x * a.x + h.x; v.y = v.y * a.y + h.y; v.z = v.z * a.z + h.z; v.w = v.w * a.w + h.w;
    }
    yr[c] = make_uint2(cv(v.x) | (cv(v.y) << 16), cv(v.z) | (cv(v.w) << 16));
  }
}

int affine_plane(const float* x, int B, int T, int C, int up, const float* scale, const float* shift, int silu,
                 void* plane, int prec, hipStream_t s) {
  if (!x || !plane || B <= 0 || T <= 0 || C <= 0 || C % 4 || up < 1 || (scale && !shift) ||
      (prec != PREC_F16 && prec != PREC_BF16) || (((uintptr_t)x) & 15) || (((uintptr_t)plane) & 7) ||
      (scale && ((((uintptr_t)scale) & 15) || (((uintptr_t)shift) & 15))) || (int64_t)B * T * up >= (1ll << 31))
    return set_error(ALCM_E_INVALID, "affine_plane: bad arguments");
  const dim3 grid((unsigned)(B * T * up)), blk(256);
  auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, blk, 0, s, x, T, C, up, scale, shift, (u16*)plane); };
  if (prec == PREC_F16) {
    if (silu) go(affine_plane_kernel<PREC_F16, true>);
    else go(affine_plane_kernel<PREC_F16, false>);
  } else {
    if (silu) go(affine_plane_kernel<PREC_BF16, true>);
    else go(affine_plane_kernel<PREC_BF16, false>);
  }
  ALCM_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- row softmax (in place)
// sim.softmax(dim=-1) (new_attention.py:121) and AttnBlock1D's softmax(dim=2) (autoencoder1d.py:270).
__global__ __launch_bounds__(256) void softmax_kernel(float* x, int rows, int n, int64_t ld) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float* xr = x + (int64_t)row * ld;
  float m = -INFINITY;
  for (int c = lane; c < n; c += 64) m = fmaxf(m, xr[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < n; c += 64) s += expf(xr[c] - m);
  s = wave_sum(s);
  const float inv = 1.0f / s;
  for (int c = lane; c < n; c += 64) xr[c] = expf(xr[c] - m) * inv;
  for (int c = n + lane; c < ld; c += 64) xr[c] = 0.f;  // zero the K-padding the P.V GEMM reads
}

int softmax_rows(float* x, int rows, int n, int64_t ld, hipStream_t s) {
  if (!x || rows <= 0 || n <= 0 || ld < n) return set_error(ALCM_E_INVALID, "softmax_rows: bad arguments");
  hipLaunchKernelGGL(softmax_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, rows, n, ld);
  ALCM_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- fused Activation1d (SnakeBeta)
// UpSample1d (resample.py:25-33) -> SnakeBeta (activations.py:107-119) -> DownSample1d
// (filter.py:86-94) in one pass, no intermediate 2T signal in HBM.
//   up[m]  = 2 * sum_{k = m+1 (mod 2)} f_up[k] * x[clamp((m + 5 - k)/2)],   m in [0, 2T)
//   s[m]   = up[m] + inv_beta[c] * sin(up[m] * alpha_exp[c])^2
//   out[j] = sum_k f_dn[k] * s[clamp(2j + k - 5, 0, 2T-1)]
// Each thread owns one channel and R consecutive outputs; the input window x[j0-6, j0+R+6)
// and the 2R+10 snake samples stay in registers (compile-time indices).  Lanes run along
// channels (coalesced).  The 12+12 filter taps are kernel arguments (SGPR operands).
constexpr int A1D_R = 16;
constexpr int A1D_W = A1D_R + 12;
constexpr int A1D_S = 2 * A1D_R + 10;

struct Taps12 {
  float up[12], dn[12];
};

// sin(x)^2 with a quadrant reduction (Cody-Waite, 3-term pi/2) and the cephes single-precision
// minimax kernels on |r| <= pi/4: ~1 ulp for |x| < 1e4, no libm call, no branches.
__device__ __forceinline__ float sin_sq(float x) {
  const float k = rintf(x * 0.63661977236758134f);
  float r = fmaf(-k, 1.5703125f, x);
  r = fmaf(-k, 4.837512969970703125e-4f, r);
  r = fmaf(-k, 7.54978995489188216e-8f, r);
  const float z = r * r;
  const float sn = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f) * z, r, r);
  const float cs = fmaf(fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z,
                                  4.166664568298827e-2f), z, -0.5f), z, 1.0f);
  const float v = (((int)k) & 1) ? cs : sn;
  return v * v;
}

__device__ __forceinline__ float snake(float u, float ea, float ib) { return u + ib * sin_sq(u * ea); }

// interior runs: every index compile-time, all values in registers
__device__ __forceinline__ void act1d_run_interior(const float* __restrict__ xb, float* __restrict__ yb, int64_t st,
                                                   int j0, float ea, float ib, const Taps12& f) {
  float win[A1D_W];
#pragma unroll
  for (int i = 0; i < A1D_W; ++i) win[i] = xb[(int64_t)(j0 - 6 + i) * st];
  float sv[A1D_S];
#pragma unroll
  for (int q = 0; q < A1D_S; ++q) {
    // m = 2*j0 - 5 + q; taps k == q (mod 2) read x[(m + 5 - k)/2] = win[(q - k)/2 + 6]
    float u = 0.f;
#pragma unroll
    for (int kk = 0; kk < 6; ++kk) {
      const int k = 2 * kk + (q & 1);
      u = fmaf(f.up[k], win[(q - k) / 2 + 6], u);
    }
    sv[q] = snake(2.0f * u, ea, ib);
  }
#pragma unroll
  for (int r = 0; r < A1D_R; ++r) {
    float o = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) o = fmaf(f.dn[k], sv[2 * r + k], o);
    yb[(int64_t)(j0 + r) * st] = o;
  }
}

// edge runs (sequence start/end, or T < R+12): direct evaluation with clamped indices, no arrays
__device__ void act1d_run_edge(const float* __restrict__ xb, float* __restrict__ yb, int T, int64_t st, int j0,
                               float ea, float ib, const Taps12& f) {
  for (int j = j0; j < j0 + A1D_R && j < T; ++j) {
    float o = 0.f;
    for (int k = 0; k < 12; ++k) {
      int m = 2 * j + k - 5;
      m = m < 0 ? 0 : (m > 2 * T - 1 ? 2 * T - 1 : m);
      float u = 0.f;
      for (int kk = 0; kk < 6; ++kk) {
        const int ku = 2 * kk + ((m & 1) ? 0 : 1);
        int xi = (m + 5 - ku) / 2;
        xi = xi < 0 ? 0 : (xi > T - 1 ? T - 1 : xi);
        u = fmaf(f.up[ku], xb[(int64_t)xi * st], u);
      }
      o = fmaf(f.dn[k], snake(2.0f * u, ea, ib), o);
    }
    yb[(int64_t)j * st] = o;
  }
}

__global__ __launch_bounds__(256) void act1d_kernel(const float* __restrict__ x, float* __restrict__ y, int T, int C,
                                                    int64_t sb, int64_t st, const float* __restrict__ aexp,
                                                    const float* __restrict__ ibeta, const Taps12 f, int runs,
                                                    uint32_t total, FastDiv cdiv, FastDiv rdiv) {
  for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < total; w += gridDim.x * 256u) {
    uint32_t rb, c, b, run;
    cdiv.divmod(w, rb, c);
    rdiv.divmod(rb, b, run);
    const int j0 = (int)run * A1D_R;
    const float* xb = x + (int64_t)b * sb + c;
    float* yb = y + (int64_t)b * sb + c;
    const float ea = aexp[c], ib = ibeta[c];
    if (j0 >= 6 && j0 + A1D_R + 6 <= T) act1d_run_interior(xb, yb, st, j0, ea, ib, f);
    else act1d_run_edge(xb, yb, T, st, j0, ea, ib, f);
  }
}

int activation1d(const float* x, float* y, int B, int T, int C, int64_t sb, int64_t st, const float* alpha_exp,
                 const float* inv_beta, const float* up_filter, const float* down_filter, hipStream_t s) {
  if (!x || !y || !alpha_exp || !inv_beta || !up_filter || !down_filter || B <= 0 || T <= 0 || C <= 0)
    return set_error(ALCM_E_INVALID, "activation1d: bad arguments");
  if (x == y) return set_error(ALCM_E_INVALID, "activation1d: in-place not supported");
  const int runs = (T + A1D_R - 1) / A1D_R;
  const int64_t total = (int64_t)B * runs * C;
  if (total >= (1ll << 31)) return set_error(ALCM_E_INVALID, "activation1d: problem too large");
  Taps12 f;
  for (int k = 0; k < 12; ++k) {
    f.up[k] = up_filter[k];
    f.dn[k] = down_filter[k];
  }
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 64);
  void* tok = prof_start(s);
  hipLaunchKernelGGL(act1d_kernel, dim3(blocks), dim3(256), 0, s, x, y, T, C, sb, st, alpha_exp, inv_beta, f, runs,
                     (uint32_t)total, FastDiv((uint32_t)C), FastDiv((uint32_t)runs));
  // per output sample: 12 up-FIR + 12 down-FIR MACs on 2 upsampled samples, 2 sin; 4 B in + 4 B out
  prof_stop(tok, s, "alcm::act1d_kernel(float const*, float*, int, int, long, long, float const*, float const*, "
            "alcm::Taps12, int, unsigned int, alcm::FastDiv, alcm::FastDiv)", 2.0 * 36.0 * B * (double)T * C,
            8.0 * B * (double)T * C);
  ALCM_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- LCM step
// LCMSampler.step, epsilon prediction (scheduling_lcm.py:465-486), same fp32 op order.
struct StepCoeffs {
  float sqrt_a, sqrt_b, c_out, c_skip, sqrt_a_prev, sqrt_b_prev;
};
// The per-element step, shared by lcm_step_kernel and lcm_step_edit_kernel: the denoised estimate of one element
// (has_u: eu is the unconditional eps of the classifier-free guidance combine, plms.py:184-186: e_u + s * (e_c - e_u))
// and the re-noised previous sample of a denoised value.  The roundings are spelled out (which products fuse into an
// fma and which are rounded on their own), so that every kernel that inlines these computes the same bits and the
// compiler's contraction choices in the surrounding code cannot change them.
__device__ __forceinline__ float lcm_denoise(float xi, float e, bool has_u, float eu, float cfg, const StepCoeffs& k) {
  if (has_u) e = fmaf(cfg, e - eu, eu);
  const float x0 = fmaf(-k.sqrt_b, e, xi) / k.sqrt_a;
  return fmaf(k.c_skip, xi, k.c_out * x0);
}
__device__ __forceinline__ float lcm_renoise(float d, float nz, const StepCoeffs& k) {
#pragma clang fp contract(off)
  const float a = k.sqrt_a_prev * d, b = k.sqrt_b_prev * nz;
  return a + b;
}

__global__ void lcm_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                const float* __restrict__ eps_u, float cfg, const float* __restrict__ noise,
                                StepCoeffs k, float* prev, float* den, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float d = lcm_denoise(x[i], eps[i], eps_u != nullptr, eps_u ? eps_u[i] : 0.f, cfg, k);
    if (den) den[i] = d;
    if (prev) prev[i] = noise ? lcm_renoise(d, noise[i], k) : d;
  }
}

int lcm_step(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise, const float* c,
             float* prev, float* den, int64_t n, hipStream_t s) {
  if (!x || !eps || !c || n < 0 || (!prev && !den)) return set_error(ALCM_E_INVALID, "lcm_step: bad arguments");
  if (n == 0) return 0;
  StepCoeffs k{c[0], c[1], c[2], c[3], c[4], c[5]};
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  void* tok = prof_start(s);
  hipLaunchKernelGGL(lcm_step_kernel, dim3(blocks), dim3(256), 0, s, x, eps, eps_u, cfg, noise, k, prev, den, n);
  // per element: x, eps (+ eps_u, + noise) in, prev and den out
  prof_stop(tok, s, "alcm::lcm_step_kernel", 8.0 * n,
            4.0 * n * (2 + (eps_u ? 1 : 0) + (noise ? 1 : 0) + (prev ? 1 : 0) + (den ? 1 : 0)));
  ALCM_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- LCM edit step and its starting point
// Latents are (B, C, T) and the mask (B, T): one work item is V consecutive frames of one clip (V = 4 with 16-byte
// accesses when T and the pointers allow, else 1) in kEditCh consecutive channel rows: the item reads the mask of its
// frames once and reuses it for its channels, whose loads are all in flight together.  Items (frames fastest, then
// channel groups, then clips) are spread over the grid with a grid-stride loop.
constexpr int kEditCh = 4;
constexpr int kEditBlock = 64;     // small blocks: the configured shapes have a few thousand items
constexpr int kEditMaxBlocks = 1024;

struct EditItem {
  int64_t b;
  int c0, t;
};
template <int V>
__device__ __forceinline__ EditItem edit_item(int64_t it, int C, int T) {
  const int TV = T / V, CG = (C + kEditCh - 1) / kEditCh;
  const int64_t row = it / TV;  // (b, channel group)
  const int64_t b = row / CG;
  return EditItem{b, (int)(row - b * CG) * kEditCh, (int)(it - row * TV) * V};
}

template <int V>
struct FVec;
template <>
struct FVec<1> {
  float v[1];
  __device__ static FVec ld(const float* p) { return FVec{{*p}}; }
  __device__ void st(float* p) const { *p = v[0]; }
};
template <>
struct FVec<4> {
  float v[4];
  __device__ static FVec ld(const float* p) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    return FVec{{f.x, f.y, f.z, f.w}};
  }
  __device__ void st(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// m = 1 keeps the step's own value and m = 0 the known one, both bit for bit; in between the blend, with both products
// rounded on their own as lcm_renoise spells its roundings out: left to the compiler, the 16-byte instantiations rounded
// both and the element ones fused the first into an fma, so a mask value whose product is inexact (0.625, not 0.25)
// gave the two access widths different bits.
__device__ __forceinline__ float mask_blend(float m, float regen, float keep) {
#pragma clang fp contract(off)
  const float a = m * regen, b = (1.f - m) * keep;
  return m == 1.f ? regen : m == 0.f ? keep : a + b;
}

template <int V>
__global__ __launch_bounds__(kEditBlock) void lcm_step_edit_kernel(
    const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ eps_u, float cfg,
    const float* __restrict__ noise, StepCoeffs k, const float* __restrict__ z0, const float* __restrict__ mask,
    float* __restrict__ prev, float* __restrict__ den, int C, int T, int64_t items) {
  for (int64_t it = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
    const EditItem w = edit_item<V>(it, C, T);
    const FVec<V> m = FVec<V>::ld(mask + w.b * T + w.t);
    const int64_t o0 = (w.b * C + w.c0) * T + w.t;
#pragma unroll
    for (int j = 0; j < kEditCh; ++j) {
      if (w.c0 + j >= C) break;
      const int64_t o = o0 + (int64_t)j * T;
      const FVec<V> xv = FVec<V>::ld(x + o), ev = FVec<V>::ld(eps + o), zv = FVec<V>::ld(z0 + o);
      FVec<V> uv = xv, nv = xv, dv, pv;
      if (eps_u) uv = FVec<V>::ld(eps_u + o);
      if (noise) nv = FVec<V>::ld(noise + o);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float d = lcm_denoise(xv.v[i], ev.v[i], eps_u != nullptr, uv.v[i], cfg, k);
        dv.v[i] = mask_blend(m.v[i], d, zv.v[i]);
        pv.v[i] = noise ? lcm_renoise(dv.v[i], nv.v[i], k) : dv.v[i];
      }
      if (den) dv.st(den + o);
      if (prev) pv.st(prev + o);
    }
  }
}

static bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if ((uintptr_t)p & 15) return false;  // NULL counts as aligned
  return true;
}
static int64_t edit_items(int B, int C, int T, bool vec) {
  return (int64_t)B * ((C + kEditCh - 1) / kEditCh) * (vec ? T / 4 : T);
}
static int edit_blocks(int64_t items) {
  return (int)std::min<int64_t>((items + kEditBlock - 1) / kEditBlock, kEditMaxBlocks);
}

int lcm_step_edit(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise, const float* c,
                  const float* z0, const float* mask, float* prev, float* den, int B, int C, int T, hipStream_t s) {
  if (!x || !eps || !c || !z0 || !mask || (!prev && !den))
    return set_error(ALCM_E_INVALID, "lcm_step_edit: null x, eps, coeffs, z0 or mask, or no output");
  if (B < 0 || C < 0 || T < 0) return set_error(ALCM_E_INVALID, "lcm_step_edit: negative B, C or T");
  if (B == 0 || C == 0 || T == 0) return 0;
  StepCoeffs k{c[0], c[1], c[2], c[3], c[4], c[5]};
  const bool vec = T % 4 == 0 && aligned16({x, eps, eps_u, noise, z0, mask, prev, den});
  const int64_t items = edit_items(B, C, T, vec);
  void* tok = prof_start(s);
  if (vec)
    hipLaunchKernelGGL(lcm_step_edit_kernel<4>, dim3(edit_blocks(items)), dim3(kEditBlock), 0, s, x, eps, eps_u, cfg,
                       noise, k, z0, mask, prev, den, C, T, items);
  else
    hipLaunchKernelGGL(lcm_step_edit_kernel<1>, dim3(edit_blocks(items)), dim3(kEditBlock), 0, s, x, eps, eps_u, cfg,
                       noise, k, z0, mask, prev, den, C, T, items);
  // per element: x, eps, z0 (+ eps_u, + noise) in, prev and den out; the mask once per frame and channel group
  const double n = (double)B * C * T;
  prof_stop(tok, s, vec ? "alcm::lcm_step_edit_kernel<4>" : "alcm::lcm_step_edit_kernel<1>", 12.0 * n,
            4.0 * n * (3 + (eps_u ? 1 : 0) + (noise ? 1 : 0) + (prev ? 1 : 0) + (den ? 1 : 0)) +
                4.0 * B * T * ((C + kEditCh - 1) / kEditCh));
  ALCM_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- joint LCM step of overlapping windows
// One long latent x (B, C, L) is covered by K windows of W frames at the frames starts[k]; the DiT ran on every window
// of every clip as one batch, eps (K * B, C, W), row k * B + b.  Per element (b, c, t), over the windows that cover t in
// ascending k: d_k = lcm_denoise(x, eps[k * B + b, c, t - s_k]); one covering window: d = d_k (a select: the plain
// step's bits); several: acc = wn[0] * d_0 rounded alone, acc = fmaf(wn[k], d_k, acc), d = acc, with wn (K, W) the
// host's normalised window weights (pipeline.joint_weights).  prev = the re-noised d, and xw (K * B, C, W) is prev
// gathered back into window layout, the next DiT input.  eps == nullptr: only x is gathered into xw, by a kernel of
// its own (joint_gather_kernel).
// Items as in the edit step: V frames of kEditCh channel rows; with V = 4 every start and W are multiples of 4, so the
// frames of one access share their covering windows.  The starts travel by value in the kernel's arguments (the window
// index is uniform, so each is a scalar load).  No atomics: an element's value is one fixed chain, whatever B, the grid
// or V.
// Ring = true (lcm_step_ring) closes the line into a ring of L frames: window k covers frame t at the offset
// t - s_k, plus L when that is negative, if it is below W (W <= L: a window covers a frame at most once).  The chain
// is the same one in ascending k, and with V = 4 an access never straddles the wrap (L, W and the starts are multiples
// of 4).
// Edit = true (lcm_step_joint_edit) blends the joint estimate with a known latent before the re-noise, as the edit step
// does: d' = mask_blend(mask[b, t], d, z0[b, c, t]), den = d', prev = the re-noised d'.  The mask is read once per item
// and the z0 rows with x and noise, ahead of the windows' loads; the other forms load nothing more than before.
// Ring and Edit together (lcm_step_ring_edit) are the ring's chain followed by that blend: a loop made from a recording.
constexpr int kJointMaxWin = 32;
struct JointStarts {
  int s[kJointMaxWin];
};
__device__ __forceinline__ float joint_first(float w, float d) {
#pragma clang fp contract(off)
  const float a = w * d;
  return a;
}
// the offset of frame t in a window that starts at s: negative or >= W when the window does not cover t
template <bool Ring>
__device__ __forceinline__ int window_offset(int t, int s, int L) {
  const int o = t - s;
  return Ring && o < 0 ? o + L : o;
}

template <int V, bool Ring, bool Edit>
__global__ __launch_bounds__(kEditBlock) void lcm_step_joint_kernel(
    const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ eps_u, float cfg,
    const float* __restrict__ noise, StepCoeffs k, JointStarts st, int K, const float* __restrict__ wn,
    const float* __restrict__ z0, const float* __restrict__ mask, float* __restrict__ prev, float* __restrict__ den,
    float* __restrict__ xw, int B, int C, int L, int W, int64_t items) {
  for (int64_t it = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
    const EditItem w = edit_item<V>(it, C, L);
    const int64_t o0 = (w.b * C + w.c0) * L + w.t;
    const int nch = C - w.c0 < kEditCh ? C - w.c0 : kEditCh;
    FVec<V> xv[kEditCh], nv[kEditCh], acc[kEditCh], one[kEditCh], zv[Edit ? kEditCh : 1], m;
    if constexpr (Edit) m = FVec<V>::ld(mask + w.b * L + w.t);
#pragma unroll
    for (int j = 0; j < kEditCh; ++j) {
      if (j >= nch) break;
      xv[j] = FVec<V>::ld(x + o0 + (int64_t)j * L);
      if (noise) nv[j] = FVec<V>::ld(noise + o0 + (int64_t)j * L);  // in flight with x, ahead of the windows' loads
      if constexpr (Edit) zv[j] = FVec<V>::ld(z0 + o0 + (int64_t)j * L);
    }
    int cover = 0;
    for (int kk = 0; kk < K; ++kk) {
      const int o = window_offset<Ring>(w.t, st.s[kk], L);
      if (o < 0 || o >= W) continue;
      const FVec<V> wv = FVec<V>::ld(wn + (int64_t)kk * W + o);
      const int64_t e0 = (((int64_t)kk * B + w.b) * C + w.c0) * W + o;
#pragma unroll
      for (int j = 0; j < kEditCh; ++j) {
        if (j >= nch) break;
        const FVec<V> ev = FVec<V>::ld(eps + e0 + (int64_t)j * W);
        FVec<V> uv = ev;
        if (eps_u) uv = FVec<V>::ld(eps_u + e0 + (int64_t)j * W);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const float d = lcm_denoise(xv[j].v[i], ev.v[i], eps_u != nullptr, uv.v[i], cfg, k);
          if (cover == 0) {
            one[j].v[i] = d;
            acc[j].v[i] = joint_first(wv.v[i], d);
          } else {
            acc[j].v[i] = fmaf(wv.v[i], d, acc[j].v[i]);
          }
        }
      }
      ++cover;
    }
    // from here on xv holds prev
#pragma unroll
    for (int j = 0; j < kEditCh; ++j) {
      if (j >= nch) break;
      const int64_t o = o0 + (int64_t)j * L;
      FVec<V> dv;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        dv.v[i] = cover == 1 ? one[j].v[i] : acc[j].v[i];
        if constexpr (Edit) dv.v[i] = mask_blend(m.v[i], dv.v[i], zv[j].v[i]);
      }
#pragma unroll
      for (int i = 0; i < V; ++i) xv[j].v[i] = noise ? lcm_renoise(dv.v[i], nv[j].v[i], k) : dv.v[i];
      if (den) dv.st(den + o);
      if (prev) xv[j].st(prev + o);
    }
    if (xw) {
      for (int kk = 0; kk < K; ++kk) {
        const int o = window_offset<Ring>(w.t, st.s[kk], L);
        if (o < 0 || o >= W) continue;
        const int64_t e0 = (((int64_t)kk * B + w.b) * C + w.c0) * W + o;
#pragma unroll
        for (int j = 0; j < kEditCh; ++j)
          if (j < nch) xv[j].st(xw + e0 + (int64_t)j * W);
      }
    }
  }
}

// the windows of the first step, cut from x: xw[k * B + b, c, t - s_k] = x[b, c, t] for every covering k
template <int V, bool Ring>
__global__ __launch_bounds__(kEditBlock) void joint_gather_kernel(const float* __restrict__ x, JointStarts st, int K,
                                                                  float* __restrict__ xw, int B, int C, int L, int W,
                                                                  int64_t items) {
  for (int64_t it = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
    const EditItem w = edit_item<V>(it, C, L);
    const int64_t o0 = (w.b * C + w.c0) * L + w.t;
    const int nch = C - w.c0 < kEditCh ? C - w.c0 : kEditCh;
    FVec<V> xv[kEditCh];
#pragma unroll
    for (int j = 0; j < kEditCh; ++j)
      if (j < nch) xv[j] = FVec<V>::ld(x + o0 + (int64_t)j * L);
    for (int kk = 0; kk < K; ++kk) {
      const int o = window_offset<Ring>(w.t, st.s[kk], L);
      if (o < 0 || o >= W) continue;
      const int64_t e0 = (((int64_t)kk * B + w.b) * C + w.c0) * W + o;
#pragma unroll
      for (int j = 0; j < kEditCh; ++j)
        if (j < nch) xv[j].st(xw + e0 + (int64_t)j * W);
    }
  }
}

// The host side of all forms.  `fn` names the entry in the errors; the open form's plan rules are those of
// pipeline.joint_weights and the ring's those of pipeline.ring_weights, checked before any launch.  Edit: the line's or
// the ring's form with z0 and mask; it has no gather-only form.
template <bool Ring, bool Edit = false>
static int step_windows(const char* fn, const float* x, const float* eps, const float* eps_u, float cfg,
                        const float* noise, const float* c, const int* starts, int K, const float* wn, const float* z0,
                        const float* mask, float* prev, float* den, float* xw, int B, int C, int L, int W,
                        hipStream_t s) {
  const std::string f = std::string(fn) + ": ";
  if (!x || !wn || !c || !starts) return set_error(ALCM_E_INVALID, f + "null x, wn, coeffs or starts");
  if (Edit && (!eps || !z0 || !mask)) return set_error(ALCM_E_INVALID, f + "null eps_cond, z0 or mask");
  if (!prev && !den && !xw) return set_error(ALCM_E_INVALID, f + "no output");
  if (!eps && (eps_u || noise || prev || den || !xw))
    return set_error(ALCM_E_INVALID, f + "without eps only x is gathered into xw");
  if (B < 0 || C < 0 || L < 0 || W < 0) return set_error(ALCM_E_INVALID, f + "negative B, C, L or W");
  if (K < (Ring ? 2 : 1) || K > kJointMaxWin)
    return set_error(ALCM_E_INVALID, f + (Ring ? "K outside 2 .. 32" : "K outside 1 .. 32"));
  if (B == 0 || C == 0 || L == 0 || W == 0) return 0;
  if (Ring && W > L) return set_error(ALCM_E_INVALID, f + "a window longer than the ring");
  JointStarts st = {};
  bool mult4 = true;
  for (int i = 0; i < K; ++i) {
    st.s[i] = starts[i];
    mult4 = mult4 && starts[i] % 4 == 0;
    if (i == 0 ? starts[0] != 0 : starts[i] <= starts[i - 1])
      return set_error(ALCM_E_INVALID, f + "starts must begin at 0 and ascend strictly");
    if (i > 0 && (int64_t)starts[i] > (int64_t)starts[i - 1] + W)
      return set_error(ALCM_E_INVALID, f + "a gap between two windows");
  }
  if (Ring) {
    if (starts[K - 1] >= L) return set_error(ALCM_E_INVALID, f + "a window starts past the ring");
    if ((int64_t)starts[K - 1] + W < L)
      return set_error(ALCM_E_INVALID, f + "a gap between the last window and the first");
  } else if ((int64_t)starts[K - 1] + W != L) {
    return set_error(ALCM_E_INVALID, f + "the last window must end at L");
  }
  StepCoeffs k{c[0], c[1], c[2], c[3], c[4], c[5]};
  const bool vec = mult4 && L % 4 == 0 && W % 4 == 0 && aligned16({x, eps, eps_u, noise, wn, z0, mask, prev, den, xw});
  const int64_t items = edit_items(B, C, L, vec);
  const dim3 grid(edit_blocks(items)), blk(kEditBlock);
  const double nl = (double)B * C * L, nw = (double)K * B * C * W;
  void* tok = prof_start(s);
  if (!Edit && !eps) {
    if (vec) hipLaunchKernelGGL((joint_gather_kernel<4, Ring>), grid, blk, 0, s, x, st, K, xw, B, C, L, W, items);
    else hipLaunchKernelGGL((joint_gather_kernel<1, Ring>), grid, blk, 0, s, x, st, K, xw, B, C, L, W, items);
    prof_stop(tok, s,
              Ring ? (vec ? "alcm::ring_gather_kernel<4>" : "alcm::ring_gather_kernel<1>")
                   : (vec ? "alcm::joint_gather_kernel<4>" : "alcm::joint_gather_kernel<1>"),
              0.0, 4.0 * (nl + nw));
    ALCM_HIP(hipGetLastError());
    return 0;
  }
  if (vec)
    hipLaunchKernelGGL((lcm_step_joint_kernel<4, Ring, Edit>), grid, blk, 0, s, x, eps, eps_u, cfg, noise, k, st, K, wn,
                       z0, mask, prev, den, xw, B, C, L, W, items);
  else
    hipLaunchKernelGGL((lcm_step_joint_kernel<1, Ring, Edit>), grid, blk, 0, s, x, eps, eps_u, cfg, noise, k, st, K, wn,
                       z0, mask, prev, den, xw, B, C, L, W, items);
  // the window tensors (eps, eps_u, xw) count K * B * C * W elements and the long ones (x, noise, prev, den, and z0 of
  // the edit form) B * C * L; the weights once per window, frame and channel group, and so the edit form's mask per
  // frame and channel group; per window element the step (8) and one multiply-add
  const int cg = (C + kEditCh - 1) / kEditCh;
  prof_stop(tok, s,
            Ring && Edit ? (vec ? "alcm::lcm_step_ring_edit_kernel<4>" : "alcm::lcm_step_ring_edit_kernel<1>")
            : Edit       ? (vec ? "alcm::lcm_step_joint_edit_kernel<4>" : "alcm::lcm_step_joint_edit_kernel<1>")
            : Ring       ? (vec ? "alcm::lcm_step_ring_kernel<4>" : "alcm::lcm_step_ring_kernel<1>")
                   : (vec ? "alcm::lcm_step_joint_kernel<4>" : "alcm::lcm_step_joint_kernel<1>"),
            10.0 * nw + (noise ? 3.0 * nl : 0.0),
            4.0 * (nl * (1 + (noise ? 1 : 0) + (prev ? 1 : 0) + (den ? 1 : 0) + (Edit ? 1 : 0)) +
                   nw * (1 + (eps_u ? 1 : 0) + (xw ? 1 : 0)) + (double)K * W * B * cg +
                   (Edit ? (double)B * L * cg : 0.0)));
  ALCM_HIP(hipGetLastError());
  return 0;
}

int lcm_step_joint(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise, const float* c,
                   const int* starts, int K, const float* wn, float* prev, float* den, float* xw, int B, int C, int L,
                   int W, hipStream_t s) {
  return step_windows<false>("lcm_step_joint", x, eps, eps_u, cfg, noise, c, starts, K, wn, nullptr, nullptr, prev, den,
                             xw, B, C, L, W, s);
}

int lcm_step_joint_edit(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise,
                        const float* c, const int* starts, int K, const float* wn, const float* z0, const float* mask,
                        float* prev, float* den, float* xw, int B, int C, int L, int W, hipStream_t s) {
  return step_windows<false, true>("lcm_step_joint_edit", x, eps, eps_u, cfg, noise, c, starts, K, wn, z0, mask, prev,
                                   den, xw, B, C, L, W, s);
}

int lcm_step_ring(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise, const float* c,
                  const int* starts, int K, const float* wn, float* prev, float* den, float* xw, int B, int C, int L,
                  int W, hipStream_t s) {
  return step_windows<true>("lcm_step_ring", x, eps, eps_u, cfg, noise, c, starts, K, wn, nullptr, nullptr, prev, den, xw,
                            B, C, L, W, s);
}

int lcm_step_ring_edit(const float* x, const float* eps, const float* eps_u, float cfg, const float* noise,
                       const float* c, const int* starts, int K, const float* wn, const float* z0, const float* mask,
                       float* prev, float* den, float* xw, int B, int C, int L, int W, hipStream_t s) {
  return step_windows<true, true>("lcm_step_ring_edit", x, eps, eps_u, cfg, noise, c, starts, K, wn, z0, mask, prev, den,
                                  xw, B, C, L, W, s);
}

// z0 = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * e0) from the encoder's (B, 2C, T) moments (the posterior mode
// scale * mean without e0; lcm_audio.py:197-204, distributions.py:24-44), or a given z0; x = the sampler's start
// sa * z0 + sb * n0 on kept frames (m = 0), sa_r * z0 + sb_r * n0 on regenerated ones (m = 1).
template <int V>
__global__ __launch_bounds__(kEditBlock) void latent_init_kernel(
    const float* __restrict__ moments, const float* __restrict__ z0_in, const float* __restrict__ e0, float scale,
    const float* __restrict__ noise, const float* __restrict__ mask, float sa, float sb, float sa_r, float sb_r,
    float* __restrict__ z0_out, float* __restrict__ x_out, int C, int T, int64_t items) {
  for (int64_t it = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
    const EditItem w = edit_item<V>(it, C, T);
    FVec<V> m = {};
    if (mask) m = FVec<V>::ld(mask + w.b * T + w.t);
    const int64_t o0 = (w.b * C + w.c0) * T + w.t;        // latent element (b, c0, t)
    const int64_t om0 = (2 * w.b * C + w.c0) * T + w.t;   // its mean; the logvar is C rows further
#pragma unroll
    for (int j = 0; j < kEditCh; ++j) {
      if (w.c0 + j >= C) break;
      const int64_t o = o0 + (int64_t)j * T, om = om0 + (int64_t)j * T;
      FVec<V> z;
      if (z0_in) {
        z = FVec<V>::ld(z0_in + o);
      } else {
        z = FVec<V>::ld(moments + om);
        if (e0) {
          const FVec<V> lv = FVec<V>::ld(moments + om + (int64_t)C * T), ev = FVec<V>::ld(e0 + o);
#pragma unroll
          for (int i = 0; i < V; ++i)
            z.v[i] = scale * (z.v[i] + expf(0.5f * fminf(fmaxf(lv.v[i], -30.f), 20.f)) * ev.v[i]);
        } else {
#pragma unroll
          for (int i = 0; i < V; ++i) z.v[i] = scale * z.v[i];
        }
      }
      if (z0_out) z.st(z0_out + o);
      if (x_out) {
        const FVec<V> nv = FVec<V>::ld(noise + o);
        FVec<V> xv;
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const float keep = sa * z.v[i] + sb * nv.v[i];
          if (mask) {
            const float regen = sa_r * z.v[i] + sb_r * nv.v[i];
            xv.v[i] = m.v[i] * regen + (1.f - m.v[i]) * keep;
          } else {
            xv.v[i] = keep;
          }
        }
        xv.st(x_out + o);
      }
    }
  }
}

int latent_init(const float* moments, const float* z0_in, const float* e0, float scale, const float* noise,
                const float* mask, float sa, float sb, float sa_r, float sb_r, float* z0_out, float* x_out, int B,
                int C, int T, hipStream_t s) {
  if ((moments != nullptr) == (z0_in != nullptr))
    return set_error(ALCM_E_INVALID, "latent_init: pass exactly one of moments and z0_in");
  if (!z0_out && !x_out) return set_error(ALCM_E_INVALID, "latent_init: no output");
  if (x_out && !noise) return set_error(ALCM_E_INVALID, "latent_init: x_out needs noise");
  if (B < 0 || C < 0 || T < 0) return set_error(ALCM_E_INVALID, "latent_init: negative B, C or T");
  if (B == 0 || C == 0 || T == 0) return 0;
  if (z0_in) e0 = nullptr;
  const bool vec = T % 4 == 0 && aligned16({moments, z0_in, e0, noise, mask, z0_out, x_out});
  const int64_t items = edit_items(B, C, T, vec);
  void* tok = prof_start(s);
  if (vec)
    hipLaunchKernelGGL(latent_init_kernel<4>, dim3(edit_blocks(items)), dim3(kEditBlock), 0, s, moments, z0_in, e0,
                       scale, noise, mask, sa, sb, sa_r, sb_r, z0_out, x_out, C, T, items);
  else
    hipLaunchKernelGGL(latent_init_kernel<1>, dim3(edit_blocks(items)), dim3(kEditBlock), 0, s, moments, z0_in, e0,
                       scale, noise, mask, sa, sb, sa_r, sb_r, z0_out, x_out, C, T, items);
  const double n = (double)B * C * T;
  prof_stop(tok, s, vec ? "alcm::latent_init_kernel<4>" : "alcm::latent_init_kernel<1>", 10.0 * n,
            4.0 * n * (1 + (e0 ? 2 : 0) + (x_out ? 2 : 0) + (z0_out ? 1 : 0)) +
                (mask ? 4.0 * B * T * ((C + kEditCh - 1) / kEditCh) : 0.0));
  ALCM_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- waveform paste
// out = orig with a decoded region gen (samples gen_start .. gen_start + Ng of each clip) blended in around the
// regenerated latent frames of mask (B, T): with d the distance in samples to the nearest sample of a regenerated frame
// of the same clip, g = 1 at d = 0, ramp[d] for 0 < d < R and 0 from R on or outside gen; out is orig at g = 0 and gen at
// g = 1, both bit for bit, and orig + g * (gen - orig) in between.  One workgroup takes kPasteTile frames of one clip:
// it reads the mask of those frames and of H = ceil(R / frame_samples) frames either side into LDS, derives per frame
// the distance in frames to the nearest regenerated frame on the left and on the right, and moves V samples per thread
// and pass (V = 4 with 16-byte accesses when the sizes and pointers allow, else 1).  In place (out == orig) a sample of
// g = 0 is neither read nor written and a tile without any g > 0 ends after the mask.
// Ring = true (wave_paste_ring): orig is one period of a loop, N = T * frame_samples exactly, the mask is circular and
// gen holds the ring's samples (gen_start + i) mod N.  d is measured round the ring: the searches through s_reg index
// frames modulo T, so a regenerated frame T - 1 fades into the first samples of frame 0 and a regenerated frame 0 into
// the end of frame T - 1.  A tile's frames are f_first + i for i below f_end - f_first <= T, taken modulo T: in place
// the frames gen covers, each once.
constexpr int kPasteTile = 8;
constexpr int kPasteHalo = 16;  // frames the ramp may reach past a regenerated frame: R <= kPasteHalo * frame_samples
constexpr int kPasteBlock = 256;

//
// Law = true (wave_paste_law): the same tiling, mask search and in-place rules with another blend.  rho (B, T + 1) per
// frame edge and gam (B, T) per regenerated frame are seam_stats' tables (rho NULL: 0 everywhere; gam NULL: 1).  A
// sample of 0 < d < R takes the rho of the edge its d is measured from and the gam of the regenerated frame at that
// edge (dl + i < dr - i: the run on the left, else the one on the right); a sample of d = 0 takes its own frame's
// gam.  The thread that searches a frame's neighbours also reads their table entries into LDS.  The blend itself is
// paste_law_blend, one rounding per operation in the order written there, shared by both access widths.
__device__ __forceinline__ float paste_law_gain(float gam, float y) {
#pragma clang fp contract(off)
  return gam * y;
}
__device__ __forceinline__ float paste_law_blend(float g, float o, float y, float rho) {
#pragma clang fp contract(off)
  const float a = 1.f - g;
  const float ao = a * o, gy = g * y;
  const float s = ao + gy;
  const float aa = a * a, gg = g * g;
  const float q = aa + gg;
  const float a2 = a + a;
  const float c0 = a2 * g;
  const float c = c0 * rho;
  const float p = q + c;
  const float n = 1.f / sqrtf(p);
  return n * s;
}

// Tab: no further argument (wave_paste, wave_paste_ring) or the two tables rho and gam (wave_paste_law)
template <int V, bool Ring, class... Tab>
__global__ __launch_bounds__(kPasteBlock) void wave_paste_kernel(
    const float* orig, const float* __restrict__ gen, const float* __restrict__ mask, const float* __restrict__ ramp,
    float* out, int64_t N, int64_t Ng, int64_t gen_start, int T, int fs, int R, int H, int f_first, int f_end, int tiles,
    FastDiv fsdiv, Tab... tab) {
  constexpr bool Law = sizeof...(Tab) != 0;
  const float* const tabs[] = {tab..., nullptr, nullptr};
  const float* const rho = tabs[0];
  const float* const gam = tabs[1];
  __shared__ int s_reg[kPasteTile + 2 * kPasteHalo];
  __shared__ int s_kl[kPasteTile], s_kr[kPasteTile];
  __shared__ float s_rho[Law ? 2 : 1][kPasteTile], s_gam[Law ? 2 : 1][kPasteTile];  // [0]: the left run's, [1]: the right
  const int b = blockIdx.x / tiles;
  const int f0 = f_first + (int)(blockIdx.x - (unsigned)b * tiles) * kPasteTile;
  const bool inplace = out == orig;
  for (int i = threadIdx.x; i < kPasteTile + 2 * H; i += kPasteBlock) {
    int f = f0 - H + i;
    if constexpr (Ring) {
      f %= T;  // H may exceed T: the search then goes round more than once
      if (f < 0) f += T;
    }
    s_reg[i] = (f >= 0 && f < T) ? (mask[(int64_t)b * T + f] > 0.f) : 0;
  }
  __syncthreads();
  int live = 0;
  if (threadIdx.x < kPasteTile) {
    // frames to the nearest regenerated frame: 0 = this one, H + 1 = none within the ramp's reach
    const int c = H + threadIdx.x;
    int kl = 0, kr = 0;
    while (kl <= H && !s_reg[c - kl]) ++kl;
    while (kr <= H && !s_reg[c + kr]) ++kr;
    s_kl[threadIdx.x] = kl;
    s_kr[threadIdx.x] = kr;
    live = kl == 0 || (int64_t)(kl - 1) * fs + 1 < R || (int64_t)(kr - 1) * fs + 1 < R;
    if constexpr (Law) {
      // the entries of the nearest regenerated frame either side (kl = 0: the frame's own gam) and of the edge it ends at
      float rl = 0.f, rr = 0.f, gl = 1.f, gr = 1.f;
      int fl = f0 + (int)threadIdx.x - kl, fr = f0 + (int)threadIdx.x + kr;
      if constexpr (Ring) {
        fl %= T, fr %= T;
        if (fl < 0) fl += T;
      }
      if (kl <= H && fl >= 0 && fl < T) {
        if (gam) gl = gam[(int64_t)b * T + fl];
        if (rho) rl = rho[(int64_t)b * (T + 1) + fl + 1];  // on a ring edge T holds edge 0's value
      }
      if (kr <= H && fr >= 0 && fr < T) {
        if (gam) gr = gam[(int64_t)b * T + fr];
        if (rho) rr = rho[(int64_t)b * (T + 1) + fr];
      }
      s_rho[0][threadIdx.x] = rl, s_rho[1][threadIdx.x] = rr;
      s_gam[0][threadIdx.x] = gl, s_gam[1][threadIdx.x] = gr;
    }
  }
  if (!__syncthreads_or(live) && inplace) return;

  const int64_t n0 = (int64_t)f0 * fs, row = (int64_t)b * N;
  const uint32_t chunks = (uint32_t)kPasteTile * fs / V;
  for (uint32_t c = threadIdx.x; c < chunks; c += kPasteBlock) {
    uint32_t j, off;
    fsdiv.divmod(c * V, j, off);
    int64_t n = n0 + (int64_t)c * V;
    if constexpr (Ring) {
      if (f0 + (int)j >= f_end) break;
      if (n >= N) n -= N;  // f_end <= f_first + T < 2 T: one turn at most
    } else {
      if (n >= N) break;
    }
    const int kl = s_kl[j], kr = s_kr[j];
    // kept frame: element i is dl + i samples past the last regenerated sample on the left, dr - i before the first on
    // the right (V = 4 only with frame_samples % 4 == 0: the elements of one access share their frame)
    const int64_t dl = off + (int64_t)(kl - 1) * fs + 1, dr = (int64_t)kr * fs - off;
    // the sample's place in gen; on a ring gen goes on across the wrap (V = 4: N, Ng and gen_start are multiples of 4)
    int64_t gi = n - gen_start;
    if (Ring && gi < 0) gi += N;
    const bool in_gen = gi >= 0 && gi + V <= Ng;
    FVec<V> g;
    bool any = false;
    int right[V];  // Law: the element's d is measured from the run on the right
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int64_t d = kl == 0 ? 0 : dl + i < dr - i ? dl + i : dr - i;
      g.v[i] = !in_gen ? 0.f : d == 0 ? 1.f : d < R ? ramp[d] : 0.f;
      any |= g.v[i] != 0.f;
      if constexpr (Law) right[i] = kl != 0 && !(dl + i < dr - i);
    }
    if (!any) {
      if (!inplace) FVec<V>::ld(orig + row + n).st(out + row + n);
      continue;
    }
    const FVec<V> ov = FVec<V>::ld(orig + row + n), gv = FVec<V>::ld(gen + (int64_t)b * Ng + gi);
    FVec<V> r;
    if constexpr (Law) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float y = gam ? paste_law_gain(s_gam[right[i]][j], gv.v[i]) : gv.v[i];
        r.v[i] = g.v[i] == 1.f ? y : g.v[i] == 0.f ? ov.v[i] : paste_law_blend(g.v[i], ov.v[i], y, s_rho[right[i]][j]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i)
        r.v[i] = g.v[i] == 1.f ? gv.v[i] : g.v[i] == 0.f ? ov.v[i] : fmaf(g.v[i], gv.v[i] - ov.v[i], ov.v[i]);
    }
    r.st(out + row + n);
  }
}

// The samples of g > 0 of one launch, from a host copy of the mask (taken only while profiling).  Ring: the frames gen
// covers go on past T and are looked up modulo T, as are their neighbours; a frame gen enters twice, at its end and
// across the wrap at its start, counts both parts.
template <bool Ring>
static double wave_paste_blended(const std::vector<float>& m, int B, int64_t N, int64_t gen_start, int64_t Ng, int T,
                                 int fs, int R, int H) {
  double blended = 0;
  const int f_lo = (int)(gen_start / fs), f_hi = (int)((gen_start + Ng + fs - 1) / fs);
  const auto reg = [&](int b, int f) {
    if (Ring) f = ((f % T) + T) % T;
    return f >= 0 && f < T && m[(size_t)b * T + f] > 0.f;
  };
  for (int b = 0; b < B; ++b)
    for (int f = f_lo; f < f_hi; ++f) {
      int kl = 0, kr = 0;
      while (kl <= H && !reg(b, f - kl)) ++kl;
      while (kr <= H && !reg(b, f + kr)) ++kr;
      const int64_t lo = std::max<int64_t>((int64_t)f * fs, gen_start);
      const int64_t hi = std::min<int64_t>({(int64_t)(f + 1) * fs, gen_start + Ng, Ring ? 2 * N : N});
      // samples of the frame within R of the left neighbour, and of the right one
      const int64_t nl = std::clamp<int64_t>(R - 1 - (int64_t)(kl - 1) * fs, 0, fs);
      const int64_t nr = std::clamp<int64_t>(R - 1 - (int64_t)(kr - 1) * fs, 0, fs);
      blended += (double)std::min<int64_t>(kl == 0 ? fs : nl + nr, std::max<int64_t>(hi - lo, 0));
    }
  return blended;
}

// The argument checks of every paste and of seam_stats, under the caller's name f.  On a line gen lies inside the clip;
// on a ring N is the period exactly, gen starts inside it, is no longer than it and may go on across the wrap.
template <bool Ring>
static int paste_check(const std::string& f, const float* orig, const float* gen, const float* mask, bool has_ramp,
                       const float* out, int B, int64_t N, int64_t gen_start, int64_t Ng, int T, int fs, int R) {
  if (!orig || !out || !mask) return set_error(ALCM_E_INVALID, f + "null orig, out or mask");
  if (B < 0 || N < 0 || Ng < 0 || gen_start < 0 || T < 0 || R < 0)
    return set_error(ALCM_E_INVALID, f + "negative B, N, Ng, gen_start, T or R");
  if (fs <= 0 || fs > (1 << 20)) return set_error(ALCM_E_INVALID, f + "frame_samples outside 1 .. 2^20");
  if (Ring) {
    if ((int64_t)T * fs != N) return set_error(ALCM_E_INVALID, f + "N must be the mask's T * frame_samples, one period");
    if (Ng > N) return set_error(ALCM_E_INVALID, f + "gen is longer than the ring");
    if (N > 0 && gen_start >= N) return set_error(ALCM_E_INVALID, f + "gen starts past the ring");
  } else {
    if ((int64_t)T * fs < N) return set_error(ALCM_E_INVALID, f + "the mask's T * frame_samples is shorter than N");
    if (gen_start + Ng > N) return set_error(ALCM_E_INVALID, f + "gen reaches past the clip");
  }
  if (R > (int64_t)kPasteHalo * fs) return set_error(ALCM_E_INVALID, f + "R exceeds 16 frames");
  if ((Ng > 0 && !gen) || (R > 0 && !has_ramp)) return set_error(ALCM_E_INVALID, f + "null gen or ramp");
  return 0;
}

// The host side of every form.  law: wave_paste_law's kernel with the tables rho and gam (either may be null).
template <bool Ring>
static int paste(const float* orig, const float* gen, const float* mask, const float* ramp, float* out, int B, int64_t N,
                 int64_t gen_start, int64_t Ng, int T, int fs, int R, hipStream_t s, bool law = false,
                 const float* rho = nullptr, const float* gam = nullptr) {
  const std::string f = law ? "wave_paste_law: " : Ring ? "wave_paste_ring: " : "wave_paste: ";
  if (const int rc = paste_check<Ring>(f, orig, gen, mask, ramp != nullptr, out, B, N, gen_start, Ng, T, fs, R)) return rc;
  if (B == 0 || N == 0) return 0;
  const bool inplace = out == orig;
  if (Ng == 0) {  // nothing to blend: no launch
    if (!inplace) ALCM_HIP(hipMemcpyAsync(out, orig, sizeof(float) * B * N, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  // in place only the frames gen covers can change (on a ring counted on past T, each frame once); out of place every
  // frame is at least copied
  const int64_t fa = inplace ? gen_start / fs : 0;
  int64_t fb = inplace ? (gen_start + Ng + fs - 1) / fs : (N + fs - 1) / fs;
  if (Ring) fb = std::min<int64_t>(fb, fa + T);
  const int64_t tiles = (fb - fa + kPasteTile - 1) / kPasteTile;
  if (tiles * B >= (1ll << 31) || fb >= (1ll << 31)) return set_error(ALCM_E_INVALID, f + "problem too large");
  const int H = (R + fs - 1) / fs;
  const bool vec = fs % 4 == 0 && N % 4 == 0 && Ng % 4 == 0 && gen_start % 4 == 0 && aligned16({orig, gen, out});
  double blended = 0;
  if (prof_enabled()) {
    std::vector<float> m((size_t)B * T);
    ALCM_HIP(hipMemcpyAsync(m.data(), mask, sizeof(float) * m.size(), hipMemcpyDeviceToHost, s));
    ALCM_HIP(hipStreamSynchronize(s));
    blended = wave_paste_blended<Ring>(m, B, N, gen_start, Ng, T, fs, R, H);
  }
  void* tok = prof_start(s);
  const dim3 grid((unsigned)(tiles * B)), block(kPasteBlock);
  const FastDiv fsdiv((uint32_t)fs);
  if (law && vec)
    hipLaunchKernelGGL((wave_paste_kernel<4, Ring, const float*, const float*>), grid, block, 0, s, orig, gen, mask, ramp, out, N, Ng, gen_start,
                       T, fs, R, H, (int)fa, (int)fb, (int)tiles, fsdiv, rho, gam);
  else if (law)
    hipLaunchKernelGGL((wave_paste_kernel<1, Ring, const float*, const float*>), grid, block, 0, s, orig, gen, mask, ramp, out, N, Ng, gen_start,
                       T, fs, R, H, (int)fa, (int)fb, (int)tiles, fsdiv, rho, gam);
  else if (vec)
    hipLaunchKernelGGL((wave_paste_kernel<4, Ring>), grid, block, 0, s, orig, gen, mask, ramp, out, N, Ng, gen_start, T,
                       fs, R, H, (int)fa, (int)fb, (int)tiles, fsdiv);
  else
    hipLaunchKernelGGL((wave_paste_kernel<1, Ring>), grid, block, 0, s, orig, gen, mask, ramp, out, N, Ng, gen_start, T,
                       fs, R, H, (int)fa, (int)fb, (int)tiles, fsdiv);
  // per sample of g > 0: orig and gen in, out out; of g = 0: a copy out of place, nothing in place; the mask per frame
  prof_stop(tok, s,
            law    ? (Ring ? (vec ? "alcm::wave_paste_law_ring_kernel<4>" : "alcm::wave_paste_law_ring_kernel<1>")
                           : (vec ? "alcm::wave_paste_law_kernel<4>" : "alcm::wave_paste_law_kernel<1>"))
            : Ring ? (vec ? "alcm::wave_paste_ring_kernel<4>" : "alcm::wave_paste_ring_kernel<1>")
                   : (vec ? "alcm::wave_paste_kernel<4>" : "alcm::wave_paste_kernel<1>"),
            (law ? 16.0 : 3.0) * blended,
            4.0 * (3.0 * blended + (inplace ? 0.0 : 2.0 * ((double)B * N - blended)) + (double)tiles * B * kPasteTile));
  ALCM_HIP(hipGetLastError());
  return 0;
}

int wave_paste(const float* orig, const float* gen, const float* mask, const float* ramp, float* out, int B, int64_t N,
               int64_t gen_start, int64_t Ng, int T, int fs, int R, hipStream_t s) {
  return paste<false>(orig, gen, mask, ramp, out, B, N, gen_start, Ng, T, fs, R, s);
}

int wave_paste_ring(const float* orig, const float* gen, const float* mask, const float* ramp, float* out, int B,
                    int64_t N, int64_t gen_start, int64_t Ng, int T, int fs, int R, hipStream_t s) {
  return paste<true>(orig, gen, mask, ramp, out, B, N, gen_start, Ng, T, fs, R, s);
}

int wave_paste_law(const float* orig, const float* gen, const float* mask, const float* ramp, const float* rho,
                   const float* gam, float* out, int B, int64_t N, int64_t gen_start, int64_t Ng, int T, int fs, int R,
                   int ring, hipStream_t s) {
  return ring ? paste<true>(orig, gen, mask, ramp, out, B, N, gen_start, Ng, T, fs, R, s, true, rho, gam)
              : paste<false>(orig, gen, mask, ramp, out, B, N, gen_start, Ng, T, fs, R, s, true, rho, gam);
}

// ---------------------------------------------------------------- seam statistics
// What wave_paste_law blends by, measured where it blends (the definitions are in include/audiolcm_hip.h).  A junction
// is a frame edge e with exactly one of the frames e - 1 and e regenerated (frames outside 0 .. T count as kept on a
// line and are taken modulo T on a ring); its zone is the samples of 0 < d < R inside gen whose d the paste measures
// from that edge.  With G the samples of the kept gap the zone lies in, the paste's tie rule (dl < dr goes left, a tie
// right) gives the junction after a run d <= G / 2 and the junction before a run d <= (G + 1) / 2, both rounded down.
//   seam_sums_kernel  a workgroup per clip and edge.  The gap is searched for over ceil(2 R / frame_samples) frames:
//                     a longer one does not shorten the zone.  Thread t sums the samples d = 1 + t, 1 + t + 256, ... in
//                     rising order in fp64 (the fp32 products are exact there), a tree over LDS sums the threads in a
//                     fixed order, and thread 0 writes Sxx, Syy, Sxy and rho.  On a ring edge T is edge 0: the
//                     workgroup of edge 0 writes both.
//   seam_gain_kernel  a workgroup per clip.  Thread t takes the frames t C .. (t + 1) C - 1, C = ceil(T / 256): it
//                     notes the first and last kept frame of its segment, finds the nearest kept frame before and
//                     after the segment from the other threads' notes (round the wrap on a ring), and walks its
//                     segment once more: every regenerated frame of a run gets gam from the sums at the run's two
//                     edges, whichever segments the run spans.
// No atomics and nothing read back on the host; a clip's values depend on its own rows alone.
constexpr int kSeamBlock = 256;

template <bool Ring>
__global__ __launch_bounds__(kSeamBlock) void seam_sums_kernel(const float* __restrict__ orig,
                                                               const float* __restrict__ gen,
                                                               const float* __restrict__ mask, int64_t N, int64_t Ng,
                                                               int64_t gen_start, int T, int fs, int R, int reach,
                                                               float* __restrict__ rho, double* __restrict__ sums) {
  __shared__ double s_acc[3][kSeamBlock];
  const int E = T + 1;
  const int b = blockIdx.x / E, e = blockIdx.x - b * E;
  if (Ring && e == T) return;
  const float* mrow = mask + (int64_t)b * T;
  const auto reg = [&](int f) {
    if constexpr (Ring) {
      f %= T;
      if (f < 0) f += T;
    }
    return f >= 0 && f < T && mrow[f] > 0.f;
  };
  const bool run_left = reg(e - 1), run_right = reg(e);
  const int t = threadIdx.x;
  float* rrow = rho + (int64_t)b * E;
  double* srow = sums + (int64_t)b * E * 3;
  if (run_left == run_right) {  // no junction
    if (t == 0) {
      rrow[e] = 1.f, srow[3 * e] = srow[3 * e + 1] = srow[3 * e + 2] = 0.0;
      if (Ring && e == 0) rrow[T] = 1.f, srow[3 * T] = srow[3 * T + 1] = srow[3 * T + 2] = 0.0;
    }
    return;
  }
  int k = 0;  // kept frames from the edge on, away from the run
  if (run_left)
    while (k < reach && !reg(e + k)) ++k;
  else
    while (k < reach && !reg(e - 1 - k)) ++k;
  const int64_t G = (int64_t)k * fs;  // k = reach: none found, G >= 2 R
  const int64_t half = run_left ? G / 2 : (G + 1) / 2;
  const int64_t dmax = half < R - 1 ? half : R - 1;
  const int64_t edge = (int64_t)e * fs;
  const float* ob = orig + (int64_t)b * N;
  const float* gb = gen + (int64_t)b * Ng;
  double sxx = 0.0, syy = 0.0, sxy = 0.0;
  for (int64_t d = 1 + t; d <= dmax; d += kSeamBlock) {
    int64_t n = run_left ? edge + d - 1 : edge - d;
    if constexpr (Ring) {  // d <= G / 2 + 1 <= N: one turn at most
      if (n >= N) n -= N;
      if (n < 0) n += N;
    }
    if (n < 0 || n >= N) continue;
    int64_t gi = n - gen_start;
    if (Ring && gi < 0) gi += N;
    if (gi < 0 || gi >= Ng) continue;
    const double x = (double)ob[n], y = (double)gb[gi];
    sxx += x * x, syy += y * y, sxy += x * y;
  }
  s_acc[0][t] = sxx, s_acc[1][t] = syy, s_acc[2][t] = sxy;
  for (int w = kSeamBlock / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w) {
      s_acc[0][t] += s_acc[0][t + w];
      s_acc[1][t] += s_acc[1][t + w];
      s_acc[2][t] += s_acc[2][t + w];
    }
  }
  if (t == 0) {
    sxx = s_acc[0][0], syy = s_acc[1][0], sxy = s_acc[2][0];
    double r = 1.0;
    if (sxx > 0.0 && syy > 0.0) {
      r = sxy / (sqrt(sxx) * sqrt(syy));
      r = r < 0.0 ? 0.0 : r > 1.0 ? 1.0 : r;
    }
    rrow[e] = (float)r, srow[3 * e] = sxx, srow[3 * e + 1] = syy, srow[3 * e + 2] = sxy;
    if (Ring && e == 0) rrow[T] = (float)r, srow[3 * T] = sxx, srow[3 * T + 1] = syy, srow[3 * T + 2] = sxy;
  }
}

template <bool Ring>
__global__ __launch_bounds__(kSeamBlock) void seam_gain_kernel(const float* __restrict__ mask,
                                                               const double* __restrict__ sums, int T,
                                                               float* __restrict__ gam) {
  __shared__ int s_first[kSeamBlock], s_last[kSeamBlock];  // the segment's first and last kept frame, -1: none
  const int b = blockIdx.x, t = threadIdx.x;
  const float* mrow = mask + (int64_t)b * T;
  const double* srow = sums + (int64_t)b * (T + 1) * 3;
  float* grow = gam + (int64_t)b * T;
  const int64_t C = ((int64_t)T + kSeamBlock - 1) / kSeamBlock;
  const int lo = (int)(t * C < T ? t * C : T), hi = (int)((t + 1) * C < T ? (t + 1) * C : T);
  int first = -1, last = -1;
  for (int f = lo; f < hi; ++f)
    if (!(mrow[f] > 0.f)) {
      if (first < 0) first = f;
      last = f;
    }
  s_first[t] = first, s_last[t] = last;
  __syncthreads();
  // the nearest kept frame before the segment and after it; on a line the clip's ends stand in (edges 0 and T, whose
  // sums are zero); on a ring the search goes on round the wrap, and a ring without a kept frame has no junction
  int before = -1, after = T;
  bool have = !Ring;
  for (int u = t - 1; u >= 0; --u)
    if (s_last[u] >= 0) {
      before = s_last[u], have = true;
      break;
    }
  for (int u = t + 1; u < kSeamBlock; ++u)
    if (s_first[u] >= 0) {
      after = s_first[u], have = true;
      break;
    }
  if constexpr (Ring) {
    if (before < 0)
      for (int u = kSeamBlock - 1; u >= t; --u)
        if (s_last[u] >= 0) {
          before = s_last[u], have = true;
          break;
        }
    if (after == T)
      for (int u = 0; u <= t; ++u)
        if (s_first[u] >= 0) {
          after = s_first[u], have = true;
          break;
        }
  }
  int prev = before;
  for (int f = lo; f < hi;) {
    if (!(mrow[f] > 0.f)) {
      grow[f] = 1.f;
      prev = f++;
      continue;
    }
    int g = f;
    while (g < hi && mrow[g] > 0.f) ++g;
    const int next = g < hi ? g : after;
    float gain = 1.f;
    if (have) {
      int el = prev + 1, er = next;  // the run's edges; on a ring a kept frame exists, so prev and next are frames
      if (Ring && el == T) el = 0;
      const double sxx = srow[3 * el] + srow[3 * er], syy = srow[3 * el + 1] + srow[3 * er + 1];
      if (sxx > 0.0 && syy > 0.0) {
        const double v = sqrt(sxx / syy);
        gain = (float)(v < 0.5 ? 0.5 : v > 2.0 ? 2.0 : v);
      }
    }
    for (int q = f; q < g; ++q) grow[q] = gain;
    f = g;
  }
}

int seam_stats(const float* orig, const float* gen, const float* mask, int B, int64_t N, int64_t gen_start, int64_t Ng,
               int T, int fs, int R, int ring, float* rho, float* gam, double* sums, hipStream_t s) {
  const std::string f = "seam_stats: ";
  if (const int rc = ring ? paste_check<true>(f, orig, gen, mask, true, orig, B, N, gen_start, Ng, T, fs, R)
                          : paste_check<false>(f, orig, gen, mask, true, orig, B, N, gen_start, Ng, T, fs, R))
    return rc;
  if (!rho || !gam || !sums) return set_error(ALCM_E_INVALID, f + "null rho, gam or sums");
  if (reinterpret_cast<uintptr_t>(sums) & 7) return set_error(ALCM_E_INVALID, f + "sums is not 8-byte aligned");
  if (B == 0 || T == 0) return 0;
  if ((int64_t)B * (T + 1ll) >= (1ll << 31)) return set_error(ALCM_E_INVALID, f + "problem too large");
  const int reach = (int)((2 * (int64_t)R + fs - 1) / fs);
  const dim3 grid((unsigned)((int64_t)B * (T + 1))), block(kSeamBlock);
  const double edges = (double)B * (T + 1);
  void* tok = prof_start(s);
  if (ring)
    hipLaunchKernelGGL(seam_sums_kernel<true>, grid, block, 0, s, orig, gen, mask, N, Ng, gen_start, T, fs, R, reach, rho,
                       sums);
  else
    hipLaunchKernelGGL(seam_sums_kernel<false>, grid, block, 0, s, orig, gen, mask, N, Ng, gen_start, T, fs, R, reach,
                       rho, sums);
  // the zones' samples are not known on the host: the tables' traffic alone is counted
  prof_stop(tok, s, ring ? "alcm::seam_sums_ring_kernel" : "alcm::seam_sums_kernel", 0.0, 36.0 * edges);
  ALCM_HIP(hipGetLastError());
  tok = prof_start(s);
  if (ring)
    hipLaunchKernelGGL(seam_gain_kernel<true>, dim3(B), block, 0, s, mask, sums, T, gam);
  else
    hipLaunchKernelGGL(seam_gain_kernel<false>, dim3(B), block, 0, s, mask, sums, T, gam);
  prof_stop(tok, s, ring ? "alcm::seam_gain_ring_kernel" : "alcm::seam_gain_kernel", 0.0, 12.0 * B * T);
  ALCM_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- loop crop and seam close
// One period of N samples cut from a longer decode ext (B, Next) of the same ring, which goes on past the period's end
// with the period's start rendered once more: out[n] = ext[start + n] from n = R on, out[0] = ext[start + N] (the sample
// that follows out[N - 1] in ext, so the wrap is an adjacent pair of one waveform), and for 0 < n < R the fade
// a + ramp[n] * (b - a) from the continuation b = ext[start + N + n] to the clip's own a = ext[start + n], in
// wave_paste's fma form on wave_paste's table.  R = 0: a plain crop.  One item is V samples of one clip (V = 4 with
// 16-byte accesses when start, N, Next and the pointers allow, else 1); the ramp is read by element, so R is free.
constexpr int kLoopBlock = 256;
constexpr int kLoopMaxBlocks = 4096;

template <int V>
__global__ __launch_bounds__(kLoopBlock) void wave_loop_kernel(const float* __restrict__ ext,
                                                               const float* __restrict__ ramp, float* __restrict__ out,
                                                               int64_t Next, int64_t start, int64_t N, int R,
                                                               int64_t items) {
  const int64_t per = N / V;
  for (int64_t it = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = it / per, n = (it - b * per) * V;
    const float* row = ext + b * Next + start;
    FVec<V> a = FVec<V>::ld(row + n);
    if (n < R) {  // n + N + V - 1 < Next: start + N + R <= Next, and with V = 4 all three are multiples of 4
      const FVec<V> c = FVec<V>::ld(row + N + n);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const int64_t m = n + i;
        if (m == 0) a.v[i] = c.v[i];
        else if (m < R) a.v[i] = fmaf(ramp[m], c.v[i] - a.v[i], a.v[i]);
      }
    }
    a.st(out + b * N + n);
  }
}

int wave_loop(const float* ext, const float* ramp, float* out, int B, int64_t Next, int64_t start, int64_t N, int R,
              hipStream_t s) {
  if (!ext || !out) return set_error(ALCM_E_INVALID, "wave_loop: null ext or out");
  if (B < 0 || Next < 0 || N < 0 || R < 0) return set_error(ALCM_E_INVALID, "wave_loop: negative B, row length, N or R");
  if (start < 0) return set_error(ALCM_E_INVALID, "wave_loop: negative start");
  if (R > N) return set_error(ALCM_E_INVALID, "wave_loop: R exceeds N");
  if (start > Next || N > Next - start || R > Next - start - N)
    return set_error(ALCM_E_INVALID, "wave_loop: start + N + R reaches past the row");
  if (R > 1 && !ramp) return set_error(ALCM_E_INVALID, "wave_loop: null ramp");
  if (B == 0 || N == 0) return 0;
  const bool vec = start % 4 == 0 && N % 4 == 0 && Next % 4 == 0 && aligned16({ext, out});
  const int64_t items = (int64_t)B * (vec ? N / 4 : N);
  const int blocks = (int)std::min<int64_t>((items + kLoopBlock - 1) / kLoopBlock, kLoopMaxBlocks);
  void* tok = prof_start(s);
  if (vec)
    hipLaunchKernelGGL(wave_loop_kernel<4>, dim3(blocks), dim3(kLoopBlock), 0, s, ext, ramp, out, Next, start, N, R, items);
  else
    hipLaunchKernelGGL(wave_loop_kernel<1>, dim3(blocks), dim3(kLoopBlock), 0, s, ext, ramp, out, Next, start, N, R, items);
  // per sample one read and one write; per sample of the fade the continuation and the ramp too, and 3 FLOPs
  const double fade = (double)B * (R > 0 ? R - 1 : 0);
  prof_stop(tok, s, vec ? "alcm::wave_loop_kernel<4>" : "alcm::wave_loop_kernel<1>", 3.0 * fade,
            4.0 * (2.0 * B * N + 2.0 * fade + (R > 0 ? B : 0)));
  ALCM_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- sinusoidal embeddings
// freqs[] is the reference's own fp32 frequency table (computed on the host exactly as
// scheduling_lcm.py:103-105 / concatDiT.py:60-62 do), so the only device math is t*f and sin/cos.
__global__ void sincos_embed_kernel(const float* __restrict__ v, float vscale, const float* __restrict__ freqs, int B,
                                    int half, int cos_first, float* out) {
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < half; i += blockDim.x) {
    const float a = (v[b] * vscale) * freqs[i];
    // arguments reach ~4e3 rad: reduce modulo 2*pi in fp64 (exact enough for |a| < 1e6), then fp32
    // sin/cos on |r| <= pi, matching the reference CPU libm to ~1 ulp (fp32 OCML on the raw argument
    // differed by up to 3e-5 here)
    const double ad = (double)a;
    const double kq = rint(ad * 0.15915494309189535);
    const float r = (float)(ad - kq * 6.283185307179586);
    const float sn = sinf(r), cs = cosf(r);
    out[(int64_t)b * 2 * half + i] = cos_first ? cs : sn;
    out[(int64_t)b * 2 * half + half + i] = cos_first ? sn : cs;
  }
}
__global__ void i64_to_f32_kernel(const int64_t* t, float* o, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = (float)t[i];
}

int sincos_embedding(const float* v, float vscale, const float* freqs, int B, int half, int cos_first, float* out,
                     hipStream_t s) {
  if (!v || !freqs || !out || B <= 0 || half <= 0) return set_error(ALCM_E_INVALID, "embedding: bad arguments");
  hipLaunchKernelGGL(sincos_embed_kernel, dim3(B), dim3(128), 0, s, v, vscale, freqs, B, half, cos_first, out);
  ALCM_HIP(hipGetLastError());
  return 0;
}

int i64_to_f32(const int64_t* t, float* o, int n, hipStream_t s) {
  hipLaunchKernelGGL(i64_to_f32_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t, o, n);
  ALCM_HIP(hipGetLastError());
  return 0;
}

__global__ void fill_kernel(float* p, int64_t n, float v) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}
int fill_f32(float* p, int64_t n, float v, hipStream_t s) {
  if (n <= 0) return 0;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(fill_kernel, dim3(blocks), dim3(256), 0, s, p, n, v);
  ALCM_HIP(hipGetLastError());
  return 0;
}

// NCT (B, C, T) -> channels-last (B, T, Cp), channels C .. Cp - 1 zero: the reference-layout inputs of the DiT proj_in
// and BigVGAN conv_pre (concatDiT.py proj_in on the NCT latent, models.py:183 on the NCT mel) as the vectorised
// channel-contiguous operand of the implicit-GEMM conv instead of a stride-T gather per element.  32 x 32 tiles
// through LDS (reads coalesced along t, writes along c).
__global__ __launch_bounds__(256) void nct_to_cl_kernel(const float* __restrict__ x, int C, int T, int Cp,
                                                        float* __restrict__ y) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + ty + 8 * j, t = t0 + tx;
    tile[ty + 8 * j][tx] = (c < C && t < T) ? x[((int64_t)b * C + c) * T + t] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = t0 + ty + 8 * j, c = c0 + tx;
    if (t < T && c < Cp) y[((int64_t)b * T + t) * Cp + c] = tile[tx][ty + 8 * j];
  }
}
int nct_to_cl(const float* x, int B, int C, int T, int Cp, float* y, hipStream_t s) {
  if (!x || !y || B <= 0 || C <= 0 || T <= 0 || Cp < C) return set_error(ALCM_E_INVALID, "nct_to_cl: bad arguments");
  hipLaunchKernelGGL(nct_to_cl_kernel, dim3((T + 31) / 32, (Cp + 31) / 32, B), dim3(256), 0, s, x, C, T, Cp, y);
  ALCM_HIP(hipGetLastError());
  return 0;
}

}  // namespace alcm

// ---------------------------------------------------------------- C-ABI
extern "C" int alcm_group_norm_affine(const float* x, int B, int T, int C, int64_t sb, int64_t st, int groups,
                                      float eps, const float* gamma, const float* beta, float* scale_out,
                                      float* shift_out, alcm_stream_t stream) {
  return alcm::group_norm_affine(x, B, T, C, sb, st, groups, eps, gamma, beta, scale_out, shift_out,
                                 (hipStream_t)stream);
}
extern "C" int alcm_row_stats(const float* x, int rows, int C, int64_t ld, float eps, float* mean, float* rstd,
                              alcm_stream_t stream) {
  return alcm::row_stats(x, rows, C, ld, eps, mean, rstd, (hipStream_t)stream);
}
extern "C" int alcm_layer_norm(const float* x, int rows, int C, int64_t ld_in, float eps, const float* gamma,
                               const float* beta, const float* add, int64_t ld_add, float* y, int64_t ld_out,
                               alcm_stream_t stream) {
  return alcm::layer_norm(x, rows, C, ld_in, eps, gamma, beta, add, ld_add, y, ld_out, (hipStream_t)stream);
}
extern "C" int alcm_softmax_rows(float* x, int rows, int n, int64_t ld, alcm_stream_t stream) {
  return alcm::softmax_rows(x, rows, n, ld, (hipStream_t)stream);
}
extern "C" int alcm_activation1d(const float* x, float* y, int B, int T, int C, int64_t sb, int64_t st,
                                 const float* alpha_exp, const float* inv_beta, const float* up_filter,
                                 const float* down_filter, alcm_stream_t stream) {
  return alcm::activation1d(x, y, B, T, C, sb, st, alpha_exp, inv_beta, up_filter, down_filter, (hipStream_t)stream);
}
extern "C" int alcm_lcm_step(const float* x, const float* eps, const float* noise, const float* coeffs,
                             float* prev_out, float* denoised_out, int64_t n, alcm_stream_t stream) {
  return alcm::lcm_step(x, eps, nullptr, 1.0f, noise, coeffs, prev_out, denoised_out, n, (hipStream_t)stream);
}
extern "C" int alcm_lcm_step_cfg(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                                 const float* noise, const float* coeffs, float* prev_out, float* denoised_out,
                                 int64_t n, alcm_stream_t stream) {
  if (!eps_uncond) return alcm::set_error(ALCM_E_INVALID, "lcm_step_cfg: null eps_uncond");
  return alcm::lcm_step(x, eps_cond, eps_uncond, cfg_scale, noise, coeffs, prev_out, denoised_out, n,
                        (hipStream_t)stream);
}
extern "C" int alcm_lcm_step_edit(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                                  const float* noise, const float* coeffs, const float* z0, const float* mask,
                                  float* prev_out, float* denoised_out, int B, int C, int T, alcm_stream_t stream) {
  return alcm::lcm_step_edit(x, eps_cond, eps_uncond, cfg_scale, noise, coeffs, z0, mask, prev_out, denoised_out, B, C,
                             T, (hipStream_t)stream);
}
extern "C" int alcm_lcm_step_joint(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                                   const float* noise, const float* coeffs, const int* starts, int K, const float* wn,
                                   float* prev_out, float* denoised_out, float* xw_out, int B, int C, int L, int W,
                                   alcm_stream_t stream) {
  return alcm::lcm_step_joint(x, eps_cond, eps_uncond, cfg_scale, noise, coeffs, starts, K, wn, prev_out, denoised_out,
                              xw_out, B, C, L, W, (hipStream_t)stream);
}
extern "C" int alcm_lcm_step_joint_edit(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                                        const float* noise, const float* coeffs, const int* starts, int K,
                                        const float* wn, const float* z0, const float* mask, float* prev_out,
                                        float* denoised_out, float* xw_out, int B, int C, int L, int W,
                                        alcm_stream_t stream) {
  return alcm::lcm_step_joint_edit(x, eps_cond, eps_uncond, cfg_scale, noise, coeffs, starts, K, wn, z0, mask, prev_out,
                                   denoised_out, xw_out, B, C, L, W, (hipStream_t)stream);
}
extern "C" int alcm_lcm_step_ring(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                                  const float* noise, const float* coeffs, const int* starts, int K, const float* wn,
                                  float* prev_out, float* denoised_out, float* xw_out, int B, int C, int L, int W,
                                  alcm_stream_t stream) {
  return alcm::lcm_step_ring(x, eps_cond, eps_uncond, cfg_scale, noise, coeffs, starts, K, wn, prev_out, denoised_out,
                             xw_out, B, C, L, W, (hipStream_t)stream);
}
extern "C" int alcm_lcm_step_ring_edit(const float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                                       const float* noise, const float* coeffs, const int* starts, int K,
                                       const float* wn, const float* z0, const float* mask, float* prev_out,
                                       float* denoised_out, float* xw_out, int B, int C, int L, int W,
                                       alcm_stream_t stream) {
  return alcm::lcm_step_ring_edit(x, eps_cond, eps_uncond, cfg_scale, noise, coeffs, starts, K, wn, z0, mask, prev_out,
                                  denoised_out, xw_out, B, C, L, W, (hipStream_t)stream);
}
extern "C" int alcm_wave_loop(const float* ext, const float* ramp, float* out, int B, int64_t row_len, int64_t start,
                              int64_t N, int R, alcm_stream_t stream) {
  return alcm::wave_loop(ext, ramp, out, B, row_len, start, N, R, (hipStream_t)stream);
}
extern "C" int alcm_latent_init(const float* moments, const float* z0_in, const float* e0, float scale,
                                const float* noise, const float* mask, float sa, float sb, float sa_r, float sb_r,
                                float* z0_out, float* x_out, int B, int C, int T, alcm_stream_t stream) {
  return alcm::latent_init(moments, z0_in, e0, scale, noise, mask, sa, sb, sa_r, sb_r, z0_out, x_out, B, C, T,
                           (hipStream_t)stream);
}
extern "C" int alcm_wave_paste(const float* orig, const float* gen, const float* mask, const float* ramp, float* out,
                               int B, int64_t N, int64_t gen_start, int64_t Ng, int T, int frame_samples, int R,
                               alcm_stream_t stream) {
  return alcm::wave_paste(orig, gen, mask, ramp, out, B, N, gen_start, Ng, T, frame_samples, R, (hipStream_t)stream);
}
extern "C" int alcm_wave_paste_ring(const float* orig, const float* gen, const float* mask, const float* ramp,
                                    float* out, int B, int64_t N, int64_t gen_start, int64_t Ng, int T,
                                    int frame_samples, int R, alcm_stream_t stream) {
  return alcm::wave_paste_ring(orig, gen, mask, ramp, out, B, N, gen_start, Ng, T, frame_samples, R,
                               (hipStream_t)stream);
}
extern "C" int alcm_wave_paste_law(const float* orig, const float* gen, const float* mask, const float* ramp,
                                   const float* rho, const float* gam, float* out, int B, int64_t N, int64_t gen_start,
                                   int64_t Ng, int T, int frame_samples, int R, int ring, alcm_stream_t stream) {
  return alcm::wave_paste_law(orig, gen, mask, ramp, rho, gam, out, B, N, gen_start, Ng, T, frame_samples, R, ring,
                              (hipStream_t)stream);
}
extern "C" int alcm_seam_stats(const float* orig, const float* gen, const float* mask, int B, int64_t N,
                               int64_t gen_start, int64_t Ng, int T, int frame_samples, int R, int ring, float* rho,
                               float* gam, double* sums, alcm_stream_t stream) {
  return alcm::seam_stats(orig, gen, mask, B, N, gen_start, Ng, T, frame_samples, R, ring, rho, gam, sums,
                          (hipStream_t)stream);
}
extern "C" int alcm_sincos_embedding(const float* v, float vscale, const float* freqs, int B, int half,
                                     int cos_first, float* out, alcm_stream_t stream) {
  return alcm::sincos_embedding(v, vscale, freqs, B, half, cos_first, out, (hipStream_t)stream);
}

extern "C" int alcm_layer_norm_plane(const float* x, int rows, int C, int64_t ld, float eps, const float* gamma,
                                     const float* beta, void* plane, int prec, alcm_stream_t stream) {
  return alcm::layer_norm_plane(x, rows, C, ld, eps, gamma, beta, plane, prec, (hipStream_t)stream);
}
