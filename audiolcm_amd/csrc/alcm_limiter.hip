// Look-ahead peak limiter of a batch of mono clips (no reference counterpart: the reference writes the vocoder's
// waveform as it is).  The host plan is audiolcm_amd/limiter.py; the definition is in include/audiolcm_hip.h.
//
// Per clip: u = fl32(x g), e = |u| (or the larger of it and the oversampled copy's), r = c / e where e > c else 1,
// m[j] = min r[j .. j + La] (hold), s[n] = mean m[n - La .. n] (attack), y[n] = min(s[n], a y[n-1] + (1 - a) s[n])
// (release, y[-1] = 1), out = copysign(min(|fl32(u fl32(y))|, c), u).  m, s and y are fp64.
//
// A clip is cut into chunks of kLmChunk samples, one per thread, and into spans of kLmLanes chunks, one per workgroup:
//   lm_curve_kernel  per span: e over the span and a halo of La either side -> LDS (fp32).  Division is monotone, so
//                    min r = c / max e: the hold is a sliding maximum of e, exact in fp32, by doubling (A_k[i] = max
//                    e[i .. i + 2^k), log2(La + 1) steps, then two overlapping windows of 2^p).  m in fp64 -> LDS; its
//                    prefix sum over the tile (a thread per 12, a scan of the 256 totals) gives s[n] = (P[n + La] -
//                    P[n - 1]) / (La + 1) -> ws.  The tile's prefix starts at the tile, so a tile of ones sums
//                    exactly.  Each sample's release step is a map f(y) = min(C, A y + D), closed under composition:
//                    f2 o f1 = min(min(C2, A2 C1 + D2), A2 A1 y + A2 D1 + D2).  A thread composes its chunk's maps,
//                    a Hillis-Steele scan composes the chunks', and the span's map -> ws.
//   lm_apply_kernel  per span: y at its start is the fold of the earlier spans' maps from y = 1 in rising order (one
//                    thread, the maps staged in LDS); s of the span from ws -> LDS, the chunk maps and their scan
//                    again, every chunk run from its true start value, fl32(y) -> LDS, and the output written from
//                    it, each thread reading only the samples it writes (so y may be x).
// No atomics; the partition depends on N and La alone, so a clip's bits depend on neither B, the strides nor the other
// clips.
#include "alcm_common.h"
#include "alcm_internal.h"

#include <cmath>

namespace alcm {

constexpr int kLmChunk = 8;
constexpr int kLmLanes = 256;
constexpr int kLmSpan = kLmChunk * kLmLanes;  // 2048
constexpr int kLmSteps = 8;                   // log2(kLmLanes)
constexpr int kLmMaxLa = 1024;
constexpr int kLmTile = kLmSpan + 2 * kLmMaxLa;        // e: the span and both halos, 4096 fp32
constexpr int kLmPer = kLmTile / kLmLanes;             // 16 e per thread in a doubling step
constexpr int kLmSumN = kLmSpan + kLmMaxLa;            // m: the span and the left halo, 3072 fp64
constexpr int kLmSumChunk = kLmSumN / kLmLanes;        // 12 m per thread in the prefix sum
constexpr int kLmSumSlots = kLmSumN + kLmLanes;        // a chunk's stride in LDS is 13 doubles: ds_read_b64 conflict-free
constexpr int kLmSSlots = kLmSpan + kLmLanes;          // s: a chunk's stride is 9 doubles
constexpr int kLmFold = 2 * kLmLanes;                  // span maps staged at a time: the scan's two buffers hold them

static_assert(kLmTile * sizeof(float) <= kLmSSlots * sizeof(double), "e and s share one buffer");

__device__ __forceinline__ int lm_sum_slot(int i) { return i + i / kLmSumChunk; }
__device__ __forceinline__ int lm_s_slot(int i) { return i + i / kLmChunk; }

struct LmMap {
  double C, A, D;  // y -> min(C, A y + D)
};

// g after f
__device__ __forceinline__ LmMap lm_after(const LmMap& g, const LmMap& f) {
  return {fmin(g.C, fma(g.A, f.C, g.D)), g.A * f.A, fma(g.A, f.D, g.D)};
}

// the chunk's map from its kLmChunk values of s (valid: the samples of the chunk inside the clip)
__device__ __forceinline__ LmMap lm_chunk_map(const double* __restrict__ s, int valid, double a, double oma) {
  LmMap m = {1.0, 1.0, 0.0};  // the identity where y <= 1, and y never exceeds 1
  if (valid > 0) m = {s[0], a, oma * s[0]};
#pragma unroll
  for (int i = 1; i < kLmChunk; ++i)
    if (i < valid) {
      const double v = s[i];
      m = {fmin(v, fma(a, m.C, oma * v)), a * m.A, fma(a, m.D, oma * v)};
    }
  return m;
}

// inclusive scan of the chunk maps in rising order; out: s_f[0][.][t] = the map of chunks 0 .. t.  Ends with a barrier.
__device__ __forceinline__ void lm_scan(LmMap m, double (*s_f)[3][kLmLanes]) {
  const int t = threadIdx.x;
  s_f[0][0][t] = m.C, s_f[0][1][t] = m.A, s_f[0][2][t] = m.D;
  __syncthreads();
  int cur = 0;
  for (int j = 0; j < kLmSteps; ++j) {
    const int d = 1 << j;
    LmMap g = {s_f[cur][0][t], s_f[cur][1][t], s_f[cur][2][t]};
    if (t >= d) {
      const LmMap f = {s_f[cur][0][t - d], s_f[cur][1][t - d], s_f[cur][2][t - d]};
      g = lm_after(g, f);
    }
    s_f[cur ^ 1][0][t] = g.C, s_f[cur ^ 1][1][t] = g.A, s_f[cur ^ 1][2][t] = g.D;
    __syncthreads();
    cur ^= 1;
  }
  static_assert(kLmSteps % 2 == 0, "the scan ends in buffer 0");
}

__device__ __forceinline__ float lm_env4(const float* __restrict__ eb, int64_t p, int os, int evec, float g, float e) {
  if (os == 4) {
    float4 v;
    if (evec) {
      v = *reinterpret_cast<const float4*>(eb + 4 * p);
    } else {
      v.x = eb[4 * p], v.y = eb[4 * p + 1], v.z = eb[4 * p + 2], v.w = eb[4 * p + 3];
    }
    e = fmaxf(fmaxf(e, fmaxf(fabsf(__fmul_rn(v.x, g)), fabsf(__fmul_rn(v.y, g)))),
              fmaxf(fabsf(__fmul_rn(v.z, g)), fabsf(__fmul_rn(v.w, g))));
  } else {
    e = fmaxf(e, fabsf(__fmul_rn(eb[p], g)));
  }
  return e;
}

// e over the samples p0 .. p0 + W of the row (zero outside 0 .. N) -> s_e; p0 and W are multiples of 4
__device__ __forceinline__ void lm_load_env(const float* __restrict__ xb, const float* __restrict__ eb, int os,
                                            int64_t p0, int W, int64_t N, int vec4, int evec, float g,
                                            float* __restrict__ s_e) {
  if (vec4) {
    for (int i = 4 * threadIdx.x; i < W; i += 4 * kLmLanes) {
      const int64_t p = p0 + i;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p >= 0 && p + 3 < N) {
        v = *reinterpret_cast<const float4*>(xb + p);
      } else if (p >= 0) {
        if (p < N) v.x = xb[p];
        if (p + 1 < N) v.y = xb[p + 1];
        if (p + 2 < N) v.z = xb[p + 2];
      }
      float e[4] = {fabsf(__fmul_rn(v.x, g)), fabsf(__fmul_rn(v.y, g)), fabsf(__fmul_rn(v.z, g)),
                    fabsf(__fmul_rn(v.w, g))};
      if (eb && p >= 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (p + k < N) e[k] = lm_env4(eb, p + k, os, evec, g, e[k]);
      }
      s_e[i] = e[0], s_e[i + 1] = e[1], s_e[i + 2] = e[2], s_e[i + 3] = e[3];
    }
  } else {
    for (int i = threadIdx.x; i < W; i += kLmLanes) {
      const int64_t p = p0 + i;
      float e = 0.f;
      if (p >= 0 && p < N) {
        e = fabsf(__fmul_rn(xb[p], g));
        if (eb) e = lm_env4(eb, p, os, evec, g, e);
      }
      s_e[i] = e;
    }
  }
}

__global__ __launch_bounds__(kLmLanes) void lm_curve_kernel(const float* __restrict__ x, const float* __restrict__ env,
                                                            int os, const float* __restrict__ gain, int64_t N,
                                                            int64_t ldx, int64_t ld_env, int nspans, float ceiling,
                                                            int La, double a, int vec4, int evec,
                                                            double* __restrict__ ws_s, double* __restrict__ ws_end) {
  __shared__ __attribute__((aligned(16))) double s_buf[kLmSSlots];  // e (fp32, kLmTile), then s (fp64, padded)
  __shared__ double s_p[kLmSumSlots];
  __shared__ double s_f[2][3][kLmLanes];
  float* s_e = reinterpret_cast<float*>(s_buf);
  const int b = blockIdx.x / nspans;
  const int k = blockIdx.x - b * nspans;
  const int t = threadIdx.x;
  const int64_t n0 = (int64_t)k * kLmSpan;
  const int H = (La + 3) & ~3;        // the halo that is loaded: La rounded up, so that the tile starts 16-byte aligned
  const int W = kLmSpan + 2 * H;
  const float g = gain[b];
  lm_load_env(x + (int64_t)b * ldx, env ? env + (int64_t)b * ld_env : nullptr, os, n0 - H, W, N, vec4, evec, g, s_e);
  __syncthreads();

  // the hold: a sliding maximum of La + 1 = w samples.  After step j, s_e[i] = max e[i .. i + 2^(j+1)) where that
  // window lies inside the tile; every window read below does.
  const int w = La + 1;
  int p = 0;
  while ((2 << p) <= w) ++p;  // 2^p <= w < 2^(p+1)
  for (int j = 0; j < p; ++j) {
    const int d = 1 << j;
    float v[kLmPer];
#pragma unroll
    for (int q = 0; q < kLmPer; ++q) {
      const int i = t + q * kLmLanes;
      v[q] = 0.f;
      if (i < W) v[q] = i + d < W ? fmaxf(s_e[i], s_e[i + d]) : s_e[i];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kLmPer; ++q) {
      const int i = t + q * kLmLanes;
      if (i < W) s_e[i] = v[q];
    }
    __syncthreads();
  }
  // m over j = n0 - La .. n0 + kLmSpan - 1 (tile index i = idx + H - La), 0 past it so that the prefix sum may run on
  const int rest = w - (1 << p);
  const int nm = kLmSpan + La;
  const double c = (double)ceiling;
#pragma unroll
  for (int q = 0; q < kLmSumChunk; ++q) {
    const int idx = t + q * kLmLanes;
    double m = 0.0;
    if (idx < nm) {
      const int i = idx + H - La;
      const float e = fmaxf(s_e[i], s_e[i + rest]);
      m = e > ceiling ? c / (double)e : 1.0;
    }
    s_p[lm_sum_slot(idx)] = m;
  }
  __syncthreads();
  // inclusive prefix sum of m over the tile: a thread per kLmSumChunk, a scan of the totals
  {
    double* mine = s_p + t * (kLmSumChunk + 1);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < kLmSumChunk; ++i) acc += mine[i], mine[i] = acc;
    double* sc = &s_f[0][0][0];  // two buffers of kLmLanes
    sc[t] = acc;
    __syncthreads();
    int cur = 0;
    for (int j = 0; j < kLmSteps; ++j) {
      const int d = 1 << j;
      double v = sc[cur * kLmLanes + t];
      if (t >= d) v += sc[cur * kLmLanes + t - d];
      sc[(cur ^ 1) * kLmLanes + t] = v;
      __syncthreads();
      cur ^= 1;
    }
    if (t) {
      const double off = sc[t - 1];
#pragma unroll
      for (int i = 0; i < kLmSumChunk; ++i) mine[i] += off;
    }
  }
  __syncthreads();
  // the attack: s[n0 + q] = (P[q + La] - P[q - 1]) / w; e is dead, s takes its place
  {
    const double dw = (double)w;
    double* srow = ws_s + (int64_t)b * N;
#pragma unroll
    for (int r = 0; r < kLmChunk; ++r) {
      const int q = t + r * kLmLanes;
      const double hi = s_p[lm_sum_slot(q + La)];
      const double lo = q ? s_p[lm_sum_slot(q - 1)] : 0.0;
      const double s = (hi - lo) / dw;
      s_buf[lm_s_slot(q)] = s;
      if (n0 + q < N) srow[n0 + q] = s;
    }
  }
  __syncthreads();
  // the release: the chunk's map, the scan, the span's map
  const int64_t left = N - n0 - (int64_t)t * kLmChunk;
  const int valid = left >= kLmChunk ? kLmChunk : (left > 0 ? (int)left : 0);
  const LmMap m = lm_chunk_map(s_buf + t * (kLmChunk + 1), valid, a, 1.0 - a);
  lm_scan(m, s_f);
  if (t < 3) ws_end[(int64_t)blockIdx.x * 3 + t] = s_f[0][t][kLmLanes - 1];
}

template <bool VEC4>
__global__ __launch_bounds__(kLmLanes) void lm_apply_kernel(const float* __restrict__ x, const float* __restrict__ gain,
                                                            float* __restrict__ y, int64_t N, int64_t ldx, int64_t ldy,
                                                            int nspans, float ceiling, double a,
                                                            const double* __restrict__ ws_s,
                                                            const double* __restrict__ ws_end) {
  __shared__ double s_s[kLmSSlots];
  __shared__ double s_f[2][3][kLmLanes];
  __shared__ float s_y[kLmSSlots];
  const int b = blockIdx.x / nspans;
  const int k = blockIdx.x - b * nspans;
  const int t = threadIdx.x;
  const int64_t n0 = (int64_t)k * kLmSpan;
  const double* srow = ws_s + (int64_t)b * N;
  for (int q = t; q < kLmSpan; q += kLmLanes) s_s[lm_s_slot(q)] = n0 + q < N ? srow[n0 + q] : 1.0;
  // y at the span's start: the earlier spans' maps from y = 1 in rising order by thread 0, staged through LDS
  double y0 = 1.0;
  {
    const double* E = ws_end + (int64_t)b * nspans * 3;
    double* stage = &s_f[0][0][0];
    for (int j0 = 0; j0 < k; j0 += kLmFold) {
      const int cnt = k - j0 < kLmFold ? k - j0 : kLmFold;
      for (int i = t; i < 3 * cnt; i += kLmLanes) stage[i] = E[3 * (int64_t)j0 + i];
      __syncthreads();
      if (t == 0)
        for (int j = 0; j < cnt; ++j) y0 = fmin(stage[3 * j], fma(stage[3 * j + 1], y0, stage[3 * j + 2]));
      __syncthreads();
    }
  }
  __syncthreads();  // s is in LDS (k == 0 passes no barrier above)
  const int64_t left = N - n0 - (int64_t)t * kLmChunk;
  const int valid = left >= kLmChunk ? kLmChunk : (left > 0 ? (int)left : 0);
  const double oma = 1.0 - a;
  const double* mine = s_s + t * (kLmChunk + 1);
  lm_scan(lm_chunk_map(mine, valid, a, oma), s_f);
  if (t == 0) s_f[1][0][0] = y0;
  __syncthreads();
  double yv = s_f[1][0][0];
  if (t) yv = fmin(s_f[0][0][t - 1], fma(s_f[0][1][t - 1], yv, s_f[0][2][t - 1]));
  float* ym = s_y + t * (kLmChunk + 1);
#pragma unroll
  for (int i = 0; i < kLmChunk; ++i) {
    const double s = mine[i];
    yv = fmin(s, fma(a, yv, oma * s));
    ym[i] = (float)yv;
  }
  __syncthreads();
  const float g = gain[b];
  const float* xb = x + (int64_t)b * ldx;
  float* yb = y + (int64_t)b * ldy;
  for (int i = 4 * t; i < kLmSpan; i += 4 * kLmLanes) {
    const int64_t n = n0 + i;
    if (n >= N) break;
    const float* yl = s_y + lm_s_slot(i);  // i is a multiple of 4: the four stay inside one chunk
    if (VEC4 && n + 3 < N) {
      const float4 v = *reinterpret_cast<const float4*>(xb + n);
      const float in[4] = {v.x, v.y, v.z, v.w};
      float o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float u = __fmul_rn(in[r], g);
        const float m = fabsf(__fmul_rn(u, yl[r]));
        o[r] = copysignf(m > ceiling ? ceiling : m, u);
      }
      *reinterpret_cast<float4*>(yb + n) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      for (int r = 0; r < 4; ++r)
        if (n + r < N) {
          const float u = __fmul_rn(xb[n + r], g);
          const float m = fabsf(__fmul_rn(u, yl[r]));
          yb[n + r] = copysignf(m > ceiling ? ceiling : m, u);
        }
    }
  }
}

static int64_t lm_spans(int64_t N) { return (N + kLmSpan - 1) / kLmSpan; }

size_t limiter_workspace_bytes(int B, int64_t N, int lookahead) {
  if (B <= 0 || N <= 0 || lookahead < 0 || lookahead > kLmMaxLa) return 0;
  return sizeof(double) * (size_t)B * ((size_t)N + 3 * (size_t)lm_spans(N));
}

int limiter(const float* x, const float* env, int os, const float* gain, float* y, int B, int64_t N, int64_t ldx,
            int64_t ld_env, int64_t ldy, float ceiling, int lookahead, double release_coef, void* ws, size_t ws_bytes,
            hipStream_t s) {
  if (!x || !gain || !y) return set_error(ALCM_E_INVALID, "limiter: null x, gain or y");
  if (env && os != 1 && os != 4) return set_error(ALCM_E_INVALID, "limiter: os must be 1 or 4 with an env");
  if (B < 0 || N < 0) return set_error(ALCM_E_INVALID, "limiter: negative B or N");
  if (ldx < N || ldy < N) return set_error(ALCM_E_INVALID, "limiter: ldx or ldy < N");
  if (env && (N > (INT64_MAX >> 2) || ld_env < N * os)) return set_error(ALCM_E_INVALID, "limiter: ld_env < N * os");
  if (!(ceiling > 0.f) || !std::isfinite(ceiling))
    return set_error(ALCM_E_INVALID, "limiter: the ceiling must be a finite positive number");
  if (lookahead < 0 || lookahead > kLmMaxLa) return set_error(ALCM_E_INVALID, "limiter: lookahead outside 0 .. 1024");
  if (!(release_coef >= 0.0 && release_coef < 1.0))
    return set_error(ALCM_E_INVALID, "limiter: release_coef outside [0, 1)");
  if (B == 0 || N == 0) return 0;
  const int64_t nspans = lm_spans(N);
  if (nspans * B >= (1ll << 31)) return set_error(ALCM_E_INVALID, "limiter: problem too large");
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < limiter_workspace_bytes(B, N, lookahead))
    return set_error(ALCM_E_INVALID, "limiter: workspace null, not 8-byte aligned or smaller than "
                                     "alcm_limiter_workspace_bytes");
  if (!env) os = 1;
  double* ws_s = static_cast<double*>(ws);
  double* ws_end = ws_s + (int64_t)B * N;
  const int xvec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && ldx % 4 == 0;
  const int evec = env && (reinterpret_cast<uintptr_t>(env) & 15) == 0 && ld_env % 4 == 0;
  const int vec1 = xvec;
  const bool vec2 = xvec && (reinterpret_cast<uintptr_t>(y) & 15) == 0 && ldy % 4 == 0;
  const double samples = (double)B * (double)N;
  const unsigned grid = (unsigned)(nspans * B);

  void* tok = prof_start(s);
  hipLaunchKernelGGL(lm_curve_kernel, dim3(grid), dim3(kLmLanes), 0, s, x, env, os, gain, N, ldx, ld_env, (int)nspans,
                     ceiling, lookahead, release_coef, vec1, evec, ws_s, ws_end);
  prof_stop(tok, s, "alcm::lm_curve_kernel", 40.0 * samples, (4.0 + (env ? 4.0 * os : 0.0) + 8.0) * samples);
  ALCM_HIP(hipGetLastError());
  tok = prof_start(s);
  if (vec2)
    hipLaunchKernelGGL((lm_apply_kernel<true>), dim3(grid), dim3(kLmLanes), 0, s, x, gain, y, N, ldx, ldy, (int)nspans,
                       ceiling, release_coef, ws_s, ws_end);
  else
    hipLaunchKernelGGL((lm_apply_kernel<false>), dim3(grid), dim3(kLmLanes), 0, s, x, gain, y, N, ldx, ldy,
                       (int)nspans, ceiling, release_coef, ws_s, ws_end);
  prof_stop(tok, s, vec2 ? "alcm::lm_apply_kernel<vec4>" : "alcm::lm_apply_kernel<elem>", 20.0 * samples,
            16.0 * samples);
  ALCM_HIP(hipGetLastError());
  return 0;
}

}  // namespace alcm

extern "C" size_t alcm_limiter_workspace_bytes(int B, int64_t N, int lookahead) {
  return alcm::limiter_workspace_bytes(B, N, lookahead);
}

extern "C" int alcm_limiter(const float* x, const float* env, int os, const float* gain, float* y, int B, int64_t N,
                            int64_t ldx, int64_t ld_env, int64_t ldy, float ceiling, int lookahead,
                            double release_coef, void* ws, size_t ws_bytes, alcm_stream_t stream) {
  return alcm::limiter(x, env, os, gain, y, B, N, ldx, ld_env, ldy, ceiling, lookahead, release_coef, ws, ws_bytes,
                       (hipStream_t)stream);
}
