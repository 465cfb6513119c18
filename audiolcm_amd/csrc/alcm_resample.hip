// Band-limited rational resampler (no reference counterpart: the reference writes its 16 kHz samples under whatever
// rate the header is told).  The filter is planned on the host (audiolcm_amd/resample.py): taps[r][k], r in [0, up),
// k in [0, ntaps), and
//   y[b][n] = sum_k taps[(n * down) mod up][k] * xm[b][floor(n * down / up) + first + k],   xm = 0 outside [0, N_in)
// with xm the mean over the channels of the interleaved input x (B, N_in, channels).
//
// One workgroup of 256 threads takes kResBlock * OPT consecutive outputs of one clip.  n0 * down = q0 * up + r0 is
// divided once per workgroup in 64 bits; inside the tile output j has (r0 + j * down) = off * up + r in 32 bits, so
// its row is r and its window starts off input samples into the tile's.  The tile's input window [q0 + first,
// q0 + first + off_last + ntaps) is staged into LDS once, downmixed and zero-filled outside the clip, with element
// loads (8-byte loads for stereo at an 8-byte aligned x), so any alignment of x gives the same values.  The tap table
// stays in global memory: a tile of T outputs visits min(T, up) rows and reads each of them once, so a copy in LDS would
// be written as often as it is read; what the table is reused for is other tiles, which the L2 serves.  With up == 1
// every output uses row 0 and its taps are uniform loads.  Each output is one fmaf chain over k = 0 .. ntaps - 1 in a
// register of its own: the bits of an output depend on nothing but its window and its row.
#include "alcm_common.h"
#include "alcm_internal.h"

namespace alcm {

constexpr int kResBlock = 256;
constexpr int64_t kResLdsFloats = 12288;  // 48 KiB of window per workgroup at most

template <int OPT, bool UP1>
__global__ __launch_bounds__(kResBlock) void resample_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                             int64_t N_in, int channels, int64_t N_out, int up,
                                                             int down, const float* __restrict__ taps, int ntaps,
                                                             int first, int tiles, int vec2) {
  extern __shared__ float s_x[];
  constexpr int kTile = kResBlock * OPT;
  const int b = blockIdx.x / tiles;
  const int64_t n0 = (int64_t)(blockIdx.x - (unsigned)b * tiles) * kTile;
  const int nt = (int)(N_out - n0 < kTile ? N_out - n0 : kTile);  // outputs of this tile, >= 1
  const int64_t t0 = n0 * down;
  const int64_t q0 = t0 / up;
  const uint32_t r0 = (uint32_t)(t0 - q0 * up);
  const uint32_t off_last = (r0 + (uint32_t)(nt - 1) * (uint32_t)down) / (uint32_t)up;
  const int wlen = (int)off_last + ntaps;
  const int64_t w0 = q0 + first;
  const float inv_c = 1.0f / (float)channels;
  const float* xb = x + (int64_t)b * N_in * channels;
  for (int i = threadIdx.x; i < wlen; i += kResBlock) {
    const int64_t p = w0 + i;
    float v = 0.f;
    if (p >= 0 && p < N_in) {
      if (channels == 1) {
        v = xb[p];
      } else if (vec2) {
        const float2 t = *reinterpret_cast<const float2*>(xb + 2 * p);
        v = (t.x + t.y) * inv_c;
      } else {
        float a = xb[p * channels];
        for (int c = 1; c < channels; ++c) a += xb[p * channels + c];
        v = a * inv_c;
      }
    }
    s_x[i] = v;
  }
  __syncthreads();

  const float* row[OPT];
  const float* win[OPT];
#pragma unroll
  for (int i = 0; i < OPT; ++i) {
    const int j = threadIdx.x + i * kResBlock;
    const uint32_t t = r0 + (uint32_t)(j < nt ? j : 0) * (uint32_t)down;
    const uint32_t off = t / (uint32_t)up;
    row[i] = UP1 ? taps : taps + (int64_t)(t - off * (uint32_t)up) * ntaps;
    win[i] = s_x + off;
  }
  float acc[OPT];
#pragma unroll
  for (int i = 0; i < OPT; ++i) acc[i] = 0.f;
  for (int k = 0; k < ntaps; ++k) {
#pragma unroll
    for (int i = 0; i < OPT; ++i) acc[i] = fmaf(row[i][k], win[i][k], acc[i]);
  }
#pragma unroll
  for (int i = 0; i < OPT; ++i) {
    const int j = threadIdx.x + i * kResBlock;
    if (j < nt) y[(int64_t)b * N_out + n0 + j] = acc[i];
  }
}

template <int OPT>
static void resample_launch(bool up1, unsigned grid, size_t lds, hipStream_t s, const float* x, float* y, int64_t N_in,
                            int channels, int64_t N_out, int up, int down, const float* taps, int ntaps, int first,
                            int tiles, int vec2) {
  if (up1)
    hipLaunchKernelGGL((resample_kernel<OPT, true>), dim3(grid), dim3(kResBlock), lds, s, x, y, N_in, channels, N_out,
                       up, down, taps, ntaps, first, tiles, vec2);
  else
    hipLaunchKernelGGL((resample_kernel<OPT, false>), dim3(grid), dim3(kResBlock), lds, s, x, y, N_in, channels, N_out,
                       up, down, taps, ntaps, first, tiles, vec2);
}

int resample(const float* x, float* y, int B, int64_t N_in, int channels, int64_t N_out, int up, int down,
             const float* taps, int ntaps, int first, hipStream_t s) {
  if (!x || !y || !taps) return set_error(ALCM_E_INVALID, "resample: null x, y or taps");
  if (up < 1 || down < 1 || ntaps < 1) return set_error(ALCM_E_INVALID, "resample: up, down or ntaps < 1");
  if (channels < 1 || channels > 8) return set_error(ALCM_E_INVALID, "resample: channels outside 1 .. 8");
  if (B < 0 || N_in < 0 || N_out < 0) return set_error(ALCM_E_INVALID, "resample: negative B, N_in or N_out");
  if (N_in > (INT64_MAX - down) / up) return set_error(ALCM_E_INVALID, "resample: N_in * up overflows");
  if (N_out != (N_in * up + down - 1) / down)
    return set_error(ALCM_E_INVALID, "resample: N_out is not ceil(N_in * up / down)");
  if (B == 0 || N_in == 0) return 0;
  // the largest tile whose window fits: (up - 1 + (tile - 1) * down) / up + ntaps floats, and whose in-tile positions
  // r0 + j * down stay in 32 bits
  int opt = 0;
  int64_t win = 0;
  for (int o : {4, 2, 1}) {
    const int64_t span = (int64_t)(up - 1) + (int64_t)(kResBlock * o - 1) * down;
    win = span / up + ntaps;
    if (win <= kResLdsFloats && span < (1ll << 31)) {
      opt = o;
      break;
    }
  }
  if (!opt) return set_error(ALCM_E_INVALID, "resample: a 256-output tile's input window exceeds 48 KiB of LDS");
  const int64_t tiles = (N_out + kResBlock * opt - 1) / (kResBlock * opt);
  if (tiles * B >= (1ll << 31)) return set_error(ALCM_E_INVALID, "resample: problem too large");
  const int vec2 = channels == 2 && (reinterpret_cast<uintptr_t>(x) & 7) == 0;
  const size_t lds = sizeof(float) * (size_t)win;
  const unsigned grid = (unsigned)(tiles * B);
  void* tok = prof_start(s);
  if (opt == 4)
    resample_launch<4>(up == 1, grid, lds, s, x, y, N_in, channels, N_out, up, down, taps, ntaps, first, (int)tiles, vec2);
  else if (opt == 2)
    resample_launch<2>(up == 1, grid, lds, s, x, y, N_in, channels, N_out, up, down, taps, ntaps, first, (int)tiles, vec2);
  else
    resample_launch<1>(up == 1, grid, lds, s, x, y, N_in, channels, N_out, up, down, taps, ntaps, first, (int)tiles, vec2);
  prof_stop(tok, s, opt == 4 ? "alcm::resample_kernel<4>" : opt == 2 ? "alcm::resample_kernel<2>" : "alcm::resample_kernel<1>",
            2.0 * ntaps * (double)B * (double)N_out,
            4.0 * (double)B * ((double)N_in * channels + (double)N_out) + 4.0 * (double)up * ntaps);
  ALCM_HIP(hipGetLastError());
  return 0;
}

}  // namespace alcm

extern "C" int alcm_resample(const float* x, float* y, int B, int64_t N_in, int channels, int64_t N_out, int up,
                             int down, const float* taps, int ntaps, int first, alcm_stream_t stream) {
  return alcm::resample(x, y, B, N_in, channels, N_out, up, down, taps, ntaps, first, (hipStream_t)stream);
}
