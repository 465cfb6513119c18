// ITU-R BS.1770 loudness of a batch of mono clips, and the gain that brings them to a target (no reference
// counterpart: the reference writes the vocoder's waveform as it is).  The host plan is audiolcm_amd/loudness.py.
//
// K-weighting is a recursion over the whole clip: two biquads in cascade, transposed direct form II, state
// s = (s1, s2, t1, t2), s' = M s + u x.  It is run in parallel over time.  A clip is cut into chunks of kLdChunk
// samples, one per thread, and into spans of kLdLanes chunks, one per workgroup.  From zero state a chunk reaches the
// state z; from the state s it reaches M^kLdChunk s + z.  Every chunk map has the same matrix, so a Hillis-Steele scan
// over the workgroup's chunks needs only the powers M^(kLdChunk * 2^j), which the host supplies in float64:
//   ld_ends_kernel   per span: the chunks from zero state, the scan, the span's end state from zero state -> ws; and
//                    the span's max |x| -> ws.
//   ld_hops_kernel   per span: its true start state is the fold of the earlier spans' end states in rising order
//                    (S = M^kLdSpan S + E, one thread, the end states staged in LDS); that state enters the first
//                    chunk, the scan gives every chunk its true start state, each chunk is run again from it and
//                    writes y^2 over its samples in LDS; one wave per hop then sums the part of the hop that lies in
//                    the span (lane-strided, butterfly) -> ws.
//   ld_combine_kernel per hop: the sum of its spans' parts in rising span order; per clip: the max of the spans' peaks.
// The state, the scan and every sum are fp64 (the high pass's poles lie at 1 - 5e-3 at 48 kHz: an fp32 state loses five
// digits); x and y^2 are fp32 in LDS.  No atomics; the partition depends on N and hop alone, so a clip's bits depend
// on neither B, ld nor the other clips.  x is read twice, the second time from L2.
#include "alcm_common.h"
#include "alcm_internal.h"

#include <cmath>

namespace alcm {

constexpr int kLdChunk = 32;
constexpr int kLdLanes = 256;
constexpr int kLdSpan = kLdChunk * kLdLanes;
constexpr int kLdSteps = 8;  // log2(kLdLanes)
constexpr int kLdStride = kLdChunk + 1;  // a chunk's stride in LDS: lane t reads bank (33 t + i), conflict-free
constexpr int kLdCoefBiq = 10;           // coef: 10 biquad coefficients, kLdSteps scan matrices, M^kLdSpan
constexpr int kLdGainWave = 64;
constexpr int kLdFold = 2 * kLdLanes;    // end states staged at a time: the scan's two buffers hold 2 * kLdLanes

struct LdBiq {
  double b0, b1, b2, a1, a2, c0, c1, c2, d1, d2;
};

__device__ __forceinline__ LdBiq ld_biq(const double* __restrict__ coef) {
  return {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], coef[8], coef[9]};
}

__device__ __forceinline__ int ld_slot(int i) { return i + i / kLdChunk; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// e += P p, P 4 x 4 row-major
__device__ __forceinline__ void ld_matvec_acc(const double* __restrict__ P, const double p[4], double e[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    e[r] = fma(P[4 * r + 3], p[3], fma(P[4 * r + 2], p[2], fma(P[4 * r + 1], p[1], fma(P[4 * r], p[0], e[r]))));
}

// kLdChunk samples of one chunk through the cascade from state s; SQ: y^2 replaces each sample
template <bool SQ>
__device__ __forceinline__ void ld_run_chunk(float* __restrict__ c, const LdBiq& q, double s[4]) {
  double s1 = s[0], s2 = s[1], t1 = s[2], t2 = s[3];
#pragma unroll 8
  for (int i = 0; i < kLdChunk; ++i) {
    const double x = (double)c[i];
    const double y1 = fma(q.b0, x, s1);
    s1 = fma(q.b1, x, fma(-q.a1, y1, s2));
    s2 = fma(q.b2, x, -q.a2 * y1);
    const double y = fma(q.c0, y1, t1);
    t1 = fma(q.c1, y1, fma(-q.d1, y, t2));
    t2 = fma(q.c2, y1, -q.d2 * y);
    if (SQ) c[i] = (float)(y * y);
  }
  s[0] = s1, s[1] = s2, s[2] = t1, s[3] = t2;
}

// samples n0 .. n0 + kLdSpan of the row xb (N samples) -> s_x, zero past N; returns the thread's max |x|
__device__ __forceinline__ float ld_load_span(const float* __restrict__ xb, int64_t n0, int64_t N, int vec4,
                                              float* __restrict__ s_x) {
  float m = 0.f;
  if (vec4) {
    for (int i = 4 * threadIdx.x; i < kLdSpan; i += 4 * kLdLanes) {
      const int64_t p = n0 + i;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p + 3 < N) {
        v = *reinterpret_cast<const float4*>(xb + p);
      } else {
        if (p < N) v.x = xb[p];
        if (p + 1 < N) v.y = xb[p + 1];
        if (p + 2 < N) v.z = xb[p + 2];
      }
      float* d = s_x + ld_slot(i);  // i is a multiple of 4: the four stay inside one chunk
      d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
      m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
  } else {
    for (int i = threadIdx.x; i < kLdSpan; i += kLdLanes) {
      const int64_t p = n0 + i;
      const float v = p < N ? xb[p] : 0.f;
      s_x[ld_slot(i)] = v;
      m = fmaxf(m, fabsf(v));
    }
  }
  return m;
}

// inclusive scan of the chunk maps: in: every thread's z (thread 0's with the span's start state folded in);
// out: s_e[0][t] = the state after chunk t.  Ends with a barrier.
__device__ __forceinline__ void ld_scan(const double* __restrict__ mats, double z[4], double (*s_e)[kLdLanes][4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int r = 0; r < 4; ++r) s_e[0][t][r] = z[r];
  __syncthreads();
  int cur = 0;
  for (int j = 0; j < kLdSteps; ++j) {
    const int d = 1 << j;
    double e[4] = {s_e[cur][t][0], s_e[cur][t][1], s_e[cur][t][2], s_e[cur][t][3]};
    if (t >= d) {
      const double p[4] = {s_e[cur][t - d][0], s_e[cur][t - d][1], s_e[cur][t - d][2], s_e[cur][t - d][3]};
      ld_matvec_acc(mats + 16 * j, p, e);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) s_e[cur ^ 1][t][r] = e[r];
    __syncthreads();
    cur ^= 1;
  }
  static_assert(kLdSteps % 2 == 0, "the scan ends in buffer 0");
}

template <bool STATE>
__global__ __launch_bounds__(kLdLanes) void ld_ends_kernel(const float* __restrict__ x, int64_t N, int64_t ld,
                                                           int nspans, const double* __restrict__ coef, int vec4,
                                                           double* __restrict__ ws_end, float* __restrict__ ws_peak) {
  __shared__ float s_x[kLdLanes * kLdStride];
  __shared__ double s_e[2][kLdLanes][4];
  __shared__ float s_m[kLdLanes / ALCM_WAVE];
  const int b = blockIdx.x / nspans;
  const int k = blockIdx.x - b * nspans;
  const int t = threadIdx.x;
  const float m = wave_max(ld_load_span(x + (int64_t)b * ld, (int64_t)k * kLdSpan, N, vec4, s_x));
  if ((t & (ALCM_WAVE - 1)) == 0) s_m[t / ALCM_WAVE] = m;
  __syncthreads();
  if (ws_peak && t == 0) {
    float mm = s_m[0];
    for (int w = 1; w < kLdLanes / ALCM_WAVE; ++w) mm = fmaxf(mm, s_m[w]);
    ws_peak[blockIdx.x] = mm;
  }
  if (STATE && k + 1 < nspans) {  // the last span's end state has no reader
    const LdBiq q = ld_biq(coef);
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    ld_run_chunk<false>(s_x + t * kLdStride, q, z);
    ld_scan(coef + kLdCoefBiq, z, s_e);
    if (t < 4) ws_end[(int64_t)blockIdx.x * 4 + t] = s_e[0][kLdLanes - 1][t];
  }
}

__global__ __launch_bounds__(kLdLanes) void ld_hops_kernel(const float* __restrict__ x, int64_t N, int64_t ld,
                                                           int nspans, const double* __restrict__ coef, int vec4,
                                                           int hop, int64_t nh, int slots,
                                                           const double* __restrict__ ws_end,
                                                           double* __restrict__ ws_part) {
  __shared__ float s_x[kLdLanes * kLdStride];
  __shared__ double s_e[2][kLdLanes][4];
  const int b = blockIdx.x / nspans;
  const int k = blockIdx.x - b * nspans;
  const int t = threadIdx.x;
  const int64_t n0 = (int64_t)k * kLdSpan;
  const int64_t covered = nh * hop;  // samples in whole hops
  if (n0 >= covered) return;         // uniform: nothing of this span is summed
  ld_load_span(x + (int64_t)b * ld, n0, N, vec4, s_x);
  const LdBiq q = ld_biq(coef);
  const double* mats = coef + kLdCoefBiq;
  // the span's start state: the earlier spans' end states folded in rising order by thread 0, staged through LDS
  // kLdFold spans at a time so that the fold waits on no global load
  double S[4] = {0.0, 0.0, 0.0, 0.0};
  {
    const double* E = ws_end + (int64_t)b * nspans * 4;
    const double* Pspan = mats + 16 * kLdSteps;
    double* stage = &s_e[0][0][0];
    for (int j0 = 0; j0 < k; j0 += kLdFold) {
      const int cnt = k - j0 < kLdFold ? k - j0 : kLdFold;
      for (int i = t; i < 4 * cnt; i += kLdLanes) stage[i] = E[4 * (int64_t)j0 + i];
      __syncthreads();
      if (t == 0) {
        for (int j = 0; j < cnt; ++j) {
          double n[4] = {stage[4 * j], stage[4 * j + 1], stage[4 * j + 2], stage[4 * j + 3]};
          ld_matvec_acc(Pspan, S, n);
#pragma unroll
          for (int r = 0; r < 4; ++r) S[r] = n[r];
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();  // the span is in LDS (k == 0 passes no barrier above)
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  ld_run_chunk<false>(s_x + t * kLdStride, q, z);
  if (t == 0) ld_matvec_acc(mats, S, z);  // chunk 0 from S ends at M^kLdChunk S + z
  ld_scan(mats, z, s_e);
  double s[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) s[r] = t ? s_e[0][t - 1][r] : S[r];
  ld_run_chunk<true>(s_x + t * kLdStride, q, s);
  __syncthreads();
  // the hops that meet [n0, end): wave w takes the hops h_lo + w, h_lo + w + 4, ...
  const int64_t end = covered - n0 < kLdSpan ? covered : n0 + kLdSpan;
  const int64_t h_lo = n0 / hop, h_hi = (end - 1) / hop;
  const int lane = t & (ALCM_WAVE - 1);
  for (int64_t h = h_lo + t / ALCM_WAVE; h <= h_hi; h += kLdLanes / ALCM_WAVE) {
    const int64_t a = h * hop, e = a + hop;
    const int i0 = (int)((a > n0 ? a : n0) - n0), i1 = (int)((e < end ? e : end) - n0);
    double acc = 0.0;
    for (int i = i0 + lane; i < i1; i += ALCM_WAVE) acc += (double)s_x[ld_slot(i)];
    acc = wave_sum_f64(acc);
    if (lane == 0) ws_part[(int64_t)blockIdx.x * slots + (h - h_lo)] = acc;
  }
}

// thread (b, h): h < nh the hop's sum over its spans' parts; h == nh the clip's peak over its spans'
__global__ void ld_combine_kernel(int B, int64_t nh, int hop, int nspans, int slots, const double* __restrict__ ws_part,
                                  const float* __restrict__ ws_peak, double* __restrict__ hop_sums,
                                  float* __restrict__ peak) {
  const int64_t per = nh + 1;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)B * per) return;
  const int b = (int)(g / per);
  const int64_t h = g - (int64_t)b * per;
  if (h == nh) {
    if (!peak) return;
    float m = 0.f;
    for (int k = 0; k < nspans; ++k) m = fmaxf(m, ws_peak[(int64_t)b * nspans + k]);
    peak[b] = m;
    return;
  }
  const int64_t a = h * hop;
  const int64_t k_lo = a / kLdSpan, k_hi = (a + hop - 1) / kLdSpan;
  double acc = 0.0;
  for (int64_t k = k_lo; k <= k_hi; ++k)
    acc += ws_part[((int64_t)b * nspans + k) * slots + (h - k * kLdSpan / hop)];
  hop_sums[(int64_t)b * nh + h] = acc;
}

static int64_t ld_spans(int64_t N) { return (N + kLdSpan - 1) / kLdSpan; }
static int ld_slots(int hop) { return kLdSpan / hop + 2; }  // the hops that can meet one span

size_t loudness_workspace_bytes(int B, int64_t N, int hop) {
  if (B <= 0 || N <= 0 || hop < 1) return 0;
  const int64_t spans = (int64_t)B * ld_spans(N);
  return (size_t)spans * (sizeof(double) * (4 + (size_t)ld_slots(hop)) + sizeof(float));
}

int loudness_hops(const float* x, int B, int64_t N, int64_t ld, const double* coef, int hop, double* hop_sums,
                  float* peak, void* ws, size_t ws_bytes, hipStream_t s) {
  if (!x) return set_error(ALCM_E_INVALID, "loudness_hops: null x");
  if (!hop_sums && !peak) return set_error(ALCM_E_INVALID, "loudness_hops: neither hop_sums_out nor peak_out");
  if (hop_sums && !coef) return set_error(ALCM_E_INVALID, "loudness_hops: hop_sums_out needs coef");
  if (B < 0 || N < 0) return set_error(ALCM_E_INVALID, "loudness_hops: negative B or N");
  if (hop < 1) return set_error(ALCM_E_INVALID, "loudness_hops: hop < 1");
  if (ld < N) return set_error(ALCM_E_INVALID, "loudness_hops: ld < N");
  if (B == 0 || N == 0) return 0;
  const int64_t nspans = ld_spans(N);
  if (nspans * B >= (1ll << 31)) return set_error(ALCM_E_INVALID, "loudness_hops: problem too large");
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < loudness_workspace_bytes(B, N, hop))
    return set_error(ALCM_E_INVALID, "loudness_hops: workspace null, not 8-byte aligned or smaller than "
                                     "alcm_loudness_workspace_bytes");
  const int slots = ld_slots(hop);
  const int64_t spans = nspans * B;
  double* ws_end = static_cast<double*>(ws);
  double* ws_part = ws_end + spans * 4;
  float* ws_peak = reinterpret_cast<float*>(ws_part + spans * slots);
  const int64_t nh = hop_sums ? N / hop : 0;
  const int vec4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && ld % 4 == 0;
  const double xbytes = 4.0 * (double)B * (double)N;
  const unsigned grid = (unsigned)spans;

  void* tok = prof_start(s);
  if (hop_sums)
    hipLaunchKernelGGL((ld_ends_kernel<true>), dim3(grid), dim3(kLdLanes), 0, s, x, N, ld, (int)nspans, coef, vec4,
                       ws_end, peak ? ws_peak : nullptr);
  else
    hipLaunchKernelGGL((ld_ends_kernel<false>), dim3(grid), dim3(kLdLanes), 0, s, x, N, ld, (int)nspans, coef, vec4,
                       ws_end, ws_peak);
  prof_stop(tok, s, hop_sums ? "alcm::ld_ends_kernel<state>" : "alcm::ld_ends_kernel<peak>",
            hop_sums ? 24.0 * (double)B * (double)N : 0.0, xbytes + 36.0 * (double)spans);
  ALCM_HIP(hipGetLastError());
  if (nh > 0) {
    tok = prof_start(s);
    hipLaunchKernelGGL(ld_hops_kernel, dim3(grid), dim3(kLdLanes), 0, s, x, N, ld, (int)nspans, coef, vec4, hop, nh,
                       slots, ws_end, ws_part);
    prof_stop(tok, s, "alcm::ld_hops_kernel", 50.0 * (double)B * (double)N,
              xbytes + (32.0 + 8.0 * slots) * (double)spans);
    ALCM_HIP(hipGetLastError());
  }
  if (nh > 0 || peak) {
    const int64_t threads = (int64_t)B * (nh + 1);
    if ((threads + 255) / 256 >= (1ll << 31)) return set_error(ALCM_E_INVALID, "loudness_hops: problem too large");
    tok = prof_start(s);
    hipLaunchKernelGGL(ld_combine_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, B, nh, hop,
                       (int)nspans, slots, ws_part, ws_peak, hop_sums, peak);
    prof_stop(tok, s, "alcm::ld_combine_kernel", 0.0, 16.0 * (double)B * (double)nh + 4.0 * (double)spans);
    ALCM_HIP(hipGetLastError());
  }
  return 0;
}

// one wave per clip; every sum is a lane-strided fp64 sum and a butterfly, so it depends on the clip alone
__global__ __launch_bounds__(kLdGainWave) void ld_gain_kernel(const double* __restrict__ hs, const float* __restrict__ peak,
                                                              int64_t nh, int hop, float target, float ceiling,
                                                              float* __restrict__ lufs, float* __restrict__ gain) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t nb = nh - 3;
  const double* S = hs + (int64_t)b * nh;
  const double inv = 1.0 / (4.0 * (double)hop);
  double L = -INFINITY;
  double sum = 0.0, cnt = 0.0;
  for (int64_t j = lane; j < nb; j += kLdGainWave) {
    const double z = (S[j] + S[j + 1] + S[j + 2] + S[j + 3]) * inv;
    if (-0.691 + 10.0 * log10(z) > -70.0) sum += z, cnt += 1.0;
  }
  sum = wave_sum_f64(sum), cnt = wave_sum_f64(cnt);
  if (cnt > 0.0) {
    const double rel = -0.691 + 10.0 * log10(sum / cnt) - 10.0;
    sum = 0.0, cnt = 0.0;
    for (int64_t j = lane; j < nb; j += kLdGainWave) {
      const double z = (S[j] + S[j + 1] + S[j + 2] + S[j + 3]) * inv;
      const double l = -0.691 + 10.0 * log10(z);
      if (l > -70.0 && l > rel) sum += z, cnt += 1.0;
    }
    sum = wave_sum_f64(sum), cnt = wave_sum_f64(cnt);
    if (cnt > 0.0) L = -0.691 + 10.0 * log10(sum / cnt);
  }
  if (lane) return;
  if (lufs) lufs[b] = (float)L;
  if (!gain) return;
  float g = 1.0f;
  if (target == target && L > -INFINITY) g = (float)pow(10.0, ((double)target - L) / 20.0);
  if (ceiling > 0.f && peak) {
    const float p = peak[b];
    if (p > 0.f && __fmul_rn(p, g) > ceiling) {
      g = (float)((double)ceiling / (double)p);
      while (__fmul_rn(p, g) > ceiling) g = nextafterf(g, 0.f);
    }
  }
  gain[b] = g;
}

int loudness_gain(const double* hop_sums, const float* peak, int B, int64_t nh, int hop, float target, float ceiling,
                  float* lufs, float* gain, hipStream_t s) {
  if (!lufs && !gain) return set_error(ALCM_E_INVALID, "loudness_gain: neither lufs_out nor gain_out");
  if (B < 0 || nh < 0) return set_error(ALCM_E_INVALID, "loudness_gain: negative B or nh");
  if (hop < 1) return set_error(ALCM_E_INVALID, "loudness_gain: hop < 1");
  if (nh > 0 && !hop_sums) return set_error(ALCM_E_INVALID, "loudness_gain: null hop_sums");
  if (gain && ceiling > 0.f && !peak) return set_error(ALCM_E_INVALID, "loudness_gain: a ceiling needs peak");
  if (B == 0) return 0;
  void* tok = prof_start(s);
  hipLaunchKernelGGL(ld_gain_kernel, dim3((unsigned)B), dim3(kLdGainWave), 0, s, hop_sums, peak, nh, hop, target,
                     ceiling, lufs, gain);
  prof_stop(tok, s, "alcm::ld_gain_kernel", 0.0, (double)B * (16.0 * (double)nh + 12.0));
  ALCM_HIP(hipGetLastError());
  return 0;
}

constexpr int kWgBlock = 256;
constexpr int kWgTile = kWgBlock * 4;

template <bool VEC4>
__global__ __launch_bounds__(kWgBlock) void wave_gain_kernel(const float* __restrict__ x, const float* __restrict__ gain,
                                                             float* __restrict__ y, int64_t N, int64_t ldx, int64_t ldy,
                                                             int tiles) {
  const int b = blockIdx.x / tiles;
  const int64_t n = (int64_t)(blockIdx.x - (unsigned)b * tiles) * kWgTile + 4 * threadIdx.x;
  const float g = gain[b];
  const float* xb = x + (int64_t)b * ldx;
  float* yb = y + (int64_t)b * ldy;
  if (VEC4 && n + 3 < N) {
    float4 v = *reinterpret_cast<const float4*>(xb + n);
    v.x *= g, v.y *= g, v.z *= g, v.w *= g;
    *reinterpret_cast<float4*>(yb + n) = v;
  } else {
    for (int i = 0; i < 4; ++i)
      if (n + i < N) yb[n + i] = xb[n + i] * g;
  }
}

int wave_gain(const float* x, const float* gain, float* y, int B, int64_t N, int64_t ldx, int64_t ldy, hipStream_t s) {
  if (!x || !gain || !y) return set_error(ALCM_E_INVALID, "wave_gain: null x, gain or y");
  if (B < 0 || N < 0) return set_error(ALCM_E_INVALID, "wave_gain: negative B or N");
  if (ldx < N || ldy < N) return set_error(ALCM_E_INVALID, "wave_gain: ld < N");
  if (B == 0 || N == 0) return 0;
  const int64_t tiles = (N + kWgTile - 1) / kWgTile;
  if (tiles * B >= (1ll << 31)) return set_error(ALCM_E_INVALID, "wave_gain: problem too large");
  const bool vec4 = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0 && ldx % 4 == 0 &&
                    ldy % 4 == 0;
  void* tok = prof_start(s);
  if (vec4)
    hipLaunchKernelGGL((wave_gain_kernel<true>), dim3((unsigned)(tiles * B)), dim3(kWgBlock), 0, s, x, gain, y, N, ldx,
                       ldy, (int)tiles);
  else
    hipLaunchKernelGGL((wave_gain_kernel<false>), dim3((unsigned)(tiles * B)), dim3(kWgBlock), 0, s, x, gain, y, N, ldx,
                       ldy, (int)tiles);
  prof_stop(tok, s, vec4 ? "alcm::wave_gain_kernel<vec4>" : "alcm::wave_gain_kernel<elem>", (double)B * (double)N,
            8.0 * (double)B * (double)N + 4.0 * B);
  ALCM_HIP(hipGetLastError());
  return 0;
}

}  // namespace alcm

extern "C" size_t alcm_loudness_workspace_bytes(int B, int64_t N, int hop) {
  return alcm::loudness_workspace_bytes(B, N, hop);
}

extern "C" int alcm_loudness_hops(const float* x, int B, int64_t N, int64_t ld, const double* coef, int hop,
                                  double* hop_sums_out, float* peak_out, void* ws, size_t ws_bytes,
                                  alcm_stream_t stream) {
  return alcm::loudness_hops(x, B, N, ld, coef, hop, hop_sums_out, peak_out, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int alcm_loudness_gain(const double* hop_sums, const float* peak, int B, int64_t nh, int hop,
                                  float target_lufs, float ceiling, float* lufs_out, float* gain_out,
                                  alcm_stream_t stream) {
  return alcm::loudness_gain(hop_sums, peak, B, nh, hop, target_lufs, ceiling, lufs_out, gain_out,
                             (hipStream_t)stream);
}

extern "C" int alcm_wave_gain(const float* x, const float* gain, float* y, int B, int64_t N, int64_t ldx, int64_t ldy,
                              alcm_stream_t stream) {
  return alcm::wave_gain(x, gain, y, B, N, ldx, ldy, (hipStream_t)stream);
}
