// The operand-plane conv planner (alcm_convplan.h): one validator and one kernel choice for alcm_opconv and
// alcm_opconv_sum.  Order of preference of a single conv: lin_plane (k = 1), wconv3 (persistent, by shape), wconv2
// (two workgroups per CU), nconv (C = 24 tail), opconv_kernel's tile ladder.  alcm_opconv_dense (the BigVGAN tail
// convs on dense weights) has its own validator and choice between tconv_kernel and tconv2_kernel, dense_conv_plan.
#include "alcm_convplan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace alcm {

namespace {

constexpr int PREC_BF16 = ALCM_PREC_BF16, PREC_SPLIT = ALCM_PREC_SPLIT, PREC_F16 = ALCM_PREC_F16,
              PREC_F16W2 = ALCM_PREC_F16W2;

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
inline uintptr_t addr(const void* p) { return (uintptr_t)p; }

int fail(ConvPlan* p, const char* msg) {
  p->err = msg;
  return ALCM_E_INVALID;
}

// " T.. C.. N.. k.." behind the name under ALCM_PROF_SHAPES
void shape_suffix(ConvPlan* p, const Knobs& k, const char* fmt, int v0, int v1, int v2, int v3 = 0, int v4 = 0,
                  int v5 = 0) {
  if (!k.prof_shapes) return;
  const size_t n = std::strlen(p->name);
  std::snprintf(p->name + n, sizeof(p->name) - n, fmt, v0, v1, v2, v3, v4, v5);
}

// the operand checks every term of alcm_opconv / alcm_opconv_sum passes before any kernel is considered
// (need_out: a sum's later terms write through args[0].out)
const char* validate_term(const alcm_opconv_args& a, bool need_out) {
  const bool act = a.act_plane != nullptr;
  if (!a.a || !a.w || (need_out && !a.out && !act && !a.geglu_plane && !a.out_plane) || a.B <= 0 || a.T <= 0 ||
      a.N <= 0 || a.ksize <= 0 || a.dil <= 0)
    return "opconv: bad arguments";
  if (a.Cp <= 0 || a.Cp % 32) return "opconv: Cp must be a positive multiple of 32";
  if ((a.ksize - 1) * a.dil > OC_HALO) return "opconv: receptive field too large";
  if (a.out_stride > 0) {
    if (a.pad < 0 || a.pad > (a.ksize - 1) * a.dil || a.out_offset < 0 || a.out_offset >= a.out_stride ||
        (int64_t)(a.T - 1) * a.out_stride + a.out_offset >= a.out_rows || !a.out || a.res || a.accumulate ||
        a.out_act || a.act_plane || a.geglu_plane)
      return "opconv: bad strided-output arguments";
  } else if (2 * a.pad != (a.ksize - 1) * a.dil) {
    return "opconv: only same-length convs";
  }
  if (a.kpad < a.ksize * a.Cp || a.kpad % 32) return "opconv: kpad mismatch";
  if (a.prec < PREC_BF16 || a.prec > PREC_F16W2) return "opconv: bad prec";
  if ((addr(a.a) & 15) || (addr(a.w) & 15) || (a.a_lo_off % 8) || (a.w_lo_off % 8))
    return "opconv: operands must be 16-byte aligned";
  if (a.C <= 0 || a.C > a.Cp) return "opconv: C must be in (0, Cp]";
  if (act) {
    if (a.out_act || a.N % 2 || !a.act_alpha_exp || !a.act_inv_beta || !a.act_up_filter || !a.act_down_filter)
      return "opconv: fused activation needs out_act == 0, even N and its parameters";
    if (a.out && a.res && a.out == a.res) return "opconv: fused activation: out aliases res";
    if ((addr(a.act_plane) & 3) || (a.act_plane_lo_off % 2)) return "opconv: act_plane alignment";
    if ((a.res && (addr(a.res) & 15)) || (a.out && (addr(a.out) & 15)) || a.N % 4)
      return "opconv: fused activation needs 16-byte aligned res/out and N % 4 == 0";
  }
  return nullptr;
}

// 1x1 conv / linear on one operand plane (ALCM_LIN1: 1 = 32-deep stages in a 4-deep ring, 2 = 64-deep stages double-
// buffered, 0 = off: wconv2, -1 = by shape: the 64-deep build for plane outputs only).  Measured per step at B = 32
// (gpurun_out/r4ag): DiT q,k,v (N = 1728, plane output) 1.04 ms on wconv2 -> 0.84 (ring) / 0.75 (64-deep); DiT
// to_out (N = 576, fp32 output + residual, one round of 351 tiles, bound by its epilogue) 0.55 -> 0.62 / 0.60.
// Eligible: f16 / bf16, k = 1 without padding, Cp % 32 == 0, N % 192 == 0, no GEGLU / strided / activated /
// accumulated output.
bool plan_lin_plane(const alcm_opconv_args& a, const Knobs& k, ConvPlan* p) {
  int v = k.lin1;
  if (v < 0) {
    if (!a.out_plane) return false;
    v = 2;
  }
  if (v == 0 || (a.prec != PREC_F16 && a.prec != PREC_BF16)) return false;
  if (a.ksize != 1 || a.pad != 0 || a.out_stride > 0 || a.geglu_plane || a.out_act || a.accumulate || a.Cp % 32 ||
      a.N % SG_BN || a.kpad < a.Cp || a.kpad % 8)
    return false;
  if (a.out_plane ? (a.out || a.res) : !a.out) return false;
  const uintptr_t wplane = addr(a.w) + (a.prec == PREC_F16 ? 4 * (uintptr_t)a.w_lo_off : 0);
  if (!al16(a.a) || (wplane & 15) || !al16(a.bias) || !al16(a.res) || !al16(a.out) || (addr(a.out_plane) & 7))
    return false;
  const int64_t M = (int64_t)a.B * a.T;
  const int64_t nwg = (M + SG_BM - 1) / SG_BM * (a.N / SG_BN);
  if (M >= (1ll << 31) || nwg >= (1ll << 30) || M * a.N >= (1ll << 40)) return false;
  const bool deep = v == 2 && a.Cp % 64 == 0;
  p->kernel = CK_LIN_PLANE;
  p->BM = SG_BM; p->BN = SG_BN;
  p->kdeep = deep ? 64 : 32; p->nstage = deep ? 2 : 4;
  p->tiles_n = a.N / SG_BN;
  p->tiles = p->grid = nwg;
  std::snprintf(p->name, sizeof(p->name), "alcm::lin_plane_kernel<%d, %d, %d>", p->kdeep, p->nstage, a.prec);
  shape_suffix(p, k, " M%d N%d K%d", (int)M, a.N, a.Cp);
  return true;
}

// workgroups of the persistent wconv3 kernel: multiples of 8 (one per XCD), at most one per CU
int64_t wconv3_grid(int64_t items, int ncu, const Knobs& k) {
  const int R = (int)((items + 7) / 8);
  int grid = 8 * std::min(ncu / 8, R);
  if (k.wconv3_grid >= 8) grid = std::min(grid, k.wconv3_grid / 8 * 8);  // tests: several tiles per workgroup
  return grid;
}

// wconv3_kernel.  Eligible: fp16 / bf16 operands, Cp % 64 == 0, 3 <= k, (k-1) d <= 64, N % 192 == 0, plain fp32
// epilogue (bias, residual, scale, accumulate; no GEGLU / strided output), or the plane output
bool plan_wconv3(const alcm_opconv_args& a, int ncu, const Knobs& k, int ks, ConvPlan* p) {
  if (a.prec != PREC_F16 && a.prec != PREC_BF16) return false;
  if (a.out_act || a.out_stride > 0 || a.geglu_plane || a.Cp % 64 || a.ksize < 3 || (a.ksize - 1) * a.dil > 64 ||
      a.N % W3_BN)
    return false;
  if (a.out_plane ? (a.out || a.res || a.accumulate || (addr(a.out_plane) & 3)) : !a.out) return false;
  const int tpb = (a.T + W3_BM - 1) / W3_BM;
  const int64_t nt = (int64_t)a.B * tpb * (a.N / W3_BN);
  if (nt >= (1ll << 30) || (int64_t)a.B * a.T * a.Cp >= (1ll << 40) || (int64_t)a.B * a.T * a.N >= (1ll << 40))
    return false;
  if ((int64_t)W3_BN * a.kpad * 2 >= (1ll << 31)) return false;  // per-lane 32-bit weight-row byte offsets
  if (ks > 1 && (a.out_plane || (a.Cp / 64) % ks || (int64_t)a.N % 4 || (addr(a.ksplit_ws) & 15) ||
                 (a.bias && (addr(a.bias) & 15)) || (a.res && (addr(a.res) & 15)) || (addr(a.out) & 15)))
    return false;
  p->kernel = CK_WCONV3;
  p->BM = W3_BM; p->BN = W3_BN;
  p->tiles_per_batch = tpb;
  p->tiles_n = a.N / W3_BN;
  p->tiles = nt;
  p->n_major = 1;
  p->ksplit = ks;
  p->grid = wconv3_grid(nt * ks, ncu, k);
  // (the rocprofv3 names of the instantiations, so bench.py finds their PMC traffic in profiles/*/kernels.json)
  std::snprintf(p->name, sizeof(p->name),
                ks > 1 ? "alcm::wconv3_kernel<%d, 1, true> + ksplit_reduce" : "alcm::wconv3_kernel<%d, 1, false>",
                a.prec);
  shape_suffix(p, k, " T%d C%d N%d k%d", a.T, a.Cp, a.N, a.ksize);
  return true;
}

// wconv2 tile by shape: 256 x 96 where the weight stream dominates the per-CU fetch (k >= 7:
// the window is amortised over >= 7 taps) and there is at least one 256-row tile per CU; 128 x 192 elsewhere.
// Measured per launch (B = 32, one box): s0 C768 k11 0.946 -> 0.860 ms, s1 C384 k11
// 0.973 -> 0.934, s2 C192 k11 0.583 -> 0.559, DiT FFN-down 0.377 -> 0.358; k3 shapes equal or slower (VAE k3 +17 %)
bool wconv2_tile256(const alcm_opconv_args& a) {
  const int64_t mt = (int64_t)a.B * ((a.T + 255) / 256);
  return a.out_stride <= 0 && a.ksize >= 7 && mt * (a.N / 96) >= 256;
}

// The wide-layer kernels.  wconv2 is eligible for single-plane precisions, N a multiple of 192 (128 x 192 tiles) or
// 96 (256 x 96 tiles), Cp a multiple of 64, (k-1)d <= 64, no output activation.  false: the caller uses the narrow
// kernels (ALCM_WCONV=0: always false for plain same-length convs, the A/B reference; the strided and GEGLU
// epilogues exist only here).
bool plan_wide(const alcm_opconv_args& a, int ncu, const Knobs& k, ConvPlan* p) {
  const bool off = k.wconv <= 0;
  const bool strided = a.out_stride > 0;
  // persistent 8-wave kernel (ALCM_WCONV3: -1 by shape, 0 off, 1 wherever eligible): by shape where the 256-row
  // M tiles are >= 85 % full (BigVGAN T = 2496 / 9984 / 19968, DiT L = 467; not the VAE's T = 312, measured +15 %,
  // nor with the clips laid end to end as padded-flat rows: 2.85 vs 2.61 ms/step on wconv2)
  // A persistent grid with fewer tiles than CUs leaves CUs idle where the two-workgroup kernel's half-size tiles share
  // them: the DiT FFN down-projection (192 tiles of 256 x 192) measured 2.98 vs 2.82 ms/step (profiles/r4s)
  const int w3 = k.wconv3;
  const int mt256 = (a.T + W3_BM - 1) / W3_BM;
  const bool full = a.T * 100 >= mt256 * W3_BM * 85;
  const int64_t tiles3 = (int64_t)a.B * mt256 * (a.N / W3_BN);
  const bool fills = tiles3 >= ncu;
  // a grid that does not fill the chip: K parts where the caller gave a partial workspace (ALCM_KSPLIT=0: never), the
  // smallest part count that minimises rounds-of-items per part (e.g. the DiT FFN down-projection: 192 tiles of
  // 256 x 192 on 256 CUs, 0.75 busy; 4 parts = 768 items = 3 per CU, 0.75 of the time plus the reduction)
  int ks = 1;
  if (!off && w3 != 0 && full && !fills && !strided && !a.geglu_plane && a.N % W3_BN == 0 && a.ksplit_ws &&
      k.ksplit != 0 && !a.out_plane && a.Cp % 64 == 0)
    ks = ksplit_parts(tiles3, ncu, a.Cp / 64, (double)a.B * a.T * a.N, (double)a.ksplit_ws_floats);
  if (!off && (a.out_plane || (int64_t)a.B * a.T >= 1024) && plan_lin_plane(a, k, p)) return true;
  if (!off && w3 != 0 && !strided && !a.geglu_plane && (w3 > 0 || (full && (fills || ks > 1))) &&
      plan_wconv3(a, ncu, k, ks, p))
    return true;
  if (off && !a.geglu_plane && !strided && !a.out_plane) return false;
  if (a.prec != PREC_F16 && a.prec != PREC_BF16) return false;
  if ((a.out_act && (a.geglu_plane || strided)) || a.Cp % 64 || a.ksize < 1 || (a.ksize - 1) * a.dil > W2_HALO)
    return false;
  // N % 96: whole tiles; else (N % 4, not strided / GEGLU) 128 x 192 tiles with a partial last one (the T5 wi, N = 5632)
  const bool ragged = a.N % 96 != 0;
  if (ragged && (a.N % 4 || strided || a.geglu_plane)) return false;
  // (only where the padded last tile wastes <= 25 % of the N tiles' columns: the text encoders' T5 wi / o, N = 5632 /
  // 1024; small ragged N stay on opconv_kernel's narrower tiles)
  if (ragged && 4 * (round_up(a.N, 192) - a.N) > round_up(a.N, 192)) return false;
  // small problems: opconv_kernel's 128-row tiles fill the chip better
  if (!a.geglu_plane && !strided && !a.out_plane && (int64_t)a.B * a.T < 1024) return false;
  if (!(al16(a.bias) && al16(a.res) && al16(a.out))) return false;
  if (a.geglu_plane && (a.res || a.accumulate || (addr(a.geglu_plane) & 3))) return false;
  // wconv2 tile: 256 x 96 halves the weight bytes every tile fetches (see the kernel comment)
  const bool t256 = !ragged && wconv2_tile256(a);
  // 160-row tiles where rounds x tile rows over the two-workgroup slots of the chip drop: the VAE's T = 312 k3 convs at
  // N = 1536 (768 tiles of 128 rows = 1.5 rounds, 512 of 160 = one; 1.82 -> 1.43 ms/step); N = 768
  // (384 tiles, one round either way) stays at 128
  // (strided: the BigVGAN stage 0 / 1 upsampler phases, T = 624 / 2496 at N = 768 / 384: 1.25 / 2.5 rounds of
  // 128-row tiles -> one / two of 160-row ones; ALCM_UPS_T160=0 keeps them at 128)
  const int64_t slots = 2 * (int64_t)ncu;
  bool t160 = false;
  if (!t256 && !a.geglu_plane && (!strided || k.ups_t160) && a.N % 192 == 0) {
    const int64_t tn = a.N / 192;
    const int64_t r128 = ((int64_t)a.B * ((a.T + 127) / 128) * tn + slots - 1) / slots;
    const int64_t r160 = ((int64_t)a.B * ((a.T + 159) / 160) * tn + slots - 1) / slots;
    t160 = r160 * 160 < r128 * 128;
  }
  const int BM = t256 ? 256 : (t160 ? 160 : 128), BN = t256 ? 96 : 192;
  if (a.N % BN != 0 && !ragged) return false;  // opconv_kernel
  const int tpb = (a.T + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN;
  const int64_t tiles = (int64_t)a.B * tpb * tiles_n;
  // K parts where the grid fills less than one round of the chip's two-workgroup slots (the text towers' out-
  // projections at 2464 rows: 80-120 tiles for 512 slots; the DiT to_out): plain fp32 epilogues only, the reduction
  // applies bias / residual / scale / accumulate in part order
  // (>= 4 chunks of 64 channels per part: a part's window staging and its partial-slice epilogue are fixed costs)
  int ks2 = 1;
  if (!off && a.ksplit_ws && k.ksplit != 0 && !a.geglu_plane && !strided && !a.out_plane && !a.out_act &&
      a.N % 4 == 0) {
    ks2 = ksplit_parts(tiles, slots, a.Cp / 64, (double)a.B * a.T * a.N, (double)a.ksplit_ws_floats);
    if (ks2 > 1 && ((addr(a.ksplit_ws) & 15) || !a.out)) ks2 = 1;
  }
  if (tiles * ks2 >= (1ll << 30) || (int64_t)a.B * a.T * a.Cp >= (1ll << 40)) return false;
  p->kernel = CK_WCONV2;
  p->BM = BM; p->BN = BN;
  p->geglu = a.geglu_plane != nullptr;
  // N-tile-major order where the weight matrix is long (Cp * k >= 4096) and there are enough M tiles to share
  // an XCD's weight slice: that XCD's N tiles stay in its L2 (C768 k11 -17 %, DiT FFN -3..-10 %); M-major
  // elsewhere (the N tiles of an M tile share its input window in L2)
  // (the GEGLU up-projection, 64 M tiles x 48 N tiles of 1 MB weight slices: N-major -4 %, its M-major order
  // re-reads the weights from the Infinity Cache once per M tile, 3 GB counted per launch)
  const int tiles_m = a.B * tpb;
  p->n_major = (a.Cp * a.ksize >= 4096 && (tiles_m >= 128 || (a.geglu_plane && tiles_m >= 64)));
  p->tiles_per_batch = tpb;
  p->tiles_n = tiles_n;
  p->tiles = tiles;
  p->ksplit = ks2;
  p->grid = tiles * ks2;
  // the demangled rocprofv3 name (template defaults included), so bench.py can join the PMC passes by name
  std::snprintf(p->name, sizeof(p->name),
                ks2 > 1 ? "alcm::wconv2_kernel<%d, %s, %d, %d> + ksplit_reduce" : "alcm::wconv2_kernel<%d, %s, %d, %d>",
                a.prec, p->geglu ? "true" : "false", BM, BN);
  shape_suffix(p, k, " T%d C%d N%d k%d", a.T, a.Cp, a.N, a.ksize);
  return true;
}

// nconv_kernel.  Eligible: single-plane activations (F16 / F16W2 / BF16), N <= 96 with N % 4 == 0, Cp in {32, 64, 96},
// (k-1)d <= 64, no output activation
bool plan_nconv(const alcm_opconv_args& a, const Knobs& k, ConvPlan* p) {
  const int nck = k.nconv;  // diagnostics / A-B: ALCM_NCONV=0 uses opconv_kernel
  if (nck == 0) return false;
  if (a.prec != PREC_F16 && a.prec != PREC_F16W2 && a.prec != PREC_BF16) return false;
  if (a.out_act || a.N > 96 || a.N % 4 || (a.ksize - 1) * a.dil > NC_HALO) return false;
  // measured (scripts/microbench.py tail): faster than opconv_kernel at C = 24 only (C = 48 / 96 pad or
  // lose occupancy); ALCM_NCONV=2 forces it for every narrow shape
  if (a.Cp != 32 && nck != 2) return false;
  if (a.Cp != 32 && a.Cp != 64 && a.Cp != 96) return false;
  if (!(al16(a.bias) && al16(a.res) && al16(a.out))) return false;
  // tile configurations (rows per tile, weight ring depth) sized for >= 2 workgroups per CU where the LDS
  // allows: C = 24 -> 256 x 32, 4 buffers (36 KB, 4 workgroups per CU); C = 48 -> 256 x 64, 4 buffers (72 KB);
  // C = 96 -> 128 x 96, 3 buffers (72 KB)
  int BM, BN, NB;
  if (a.N <= 32 && a.Cp == 32) BM = 256, BN = 32, NB = 4;
  else if (a.N <= 64 && a.Cp == 64) BM = 256, BN = 64, NB = 4;
  else if (a.N <= 96 && a.Cp == 96) BM = 128, BN = 96, NB = 3;
  else return false;
  const bool act = a.act_plane != nullptr;
  const int tstride = act ? BM - 2 * ACT_EPI_HALO : BM;
  const int tpb = (a.T + tstride - 1) / tstride;
  const int64_t nwg = (int64_t)a.B * tpb;
  if (nwg >= (1ll << 31)) return false;
  p->kernel = CK_NCONV;
  p->BM = BM; p->BN = BN; p->nstage = NB;
  p->act = act;
  p->tiles_per_batch = tpb;
  p->tiles_n = 1;
  p->tiles = p->grid = nwg;
  // the demangled rocprofv3 name of the instantiation
  std::snprintf(p->name, sizeof(p->name), "alcm::nconv_kernel<%d, %d, %d, %d, %d, %s>", BM, BN, a.Cp / 32, NB, a.prec,
                act ? "true" : "false");
  return true;
}

// opconv_kernel's tile ladder
int plan_opconv_kernel(const alcm_opconv_args& a, const Knobs& k, ConvPlan* p) {
  const bool act = a.act_plane != nullptr;
  const int N = a.N;
  // one tap per K step (two taps per step measured slower: the larger weight buffers cost occupancy)
  // small problems whose 128 x 128 tiles would leave CUs idle (the text encoders' N = 1024 projections at
  // M = 2464: 160 tiles for 256 CUs) take the 96-column tiles (220 tiles): text encode 13.5 -> 13.2 ms per B = 32
  // (profiles/r3v); ALCM_OPCONV_TILE=-1 keeps the 128 x 128 tiles (A/B)
  const int64_t tiles128 = (int64_t)a.B * ((a.T + 127) / 128) * ((N + 127) / 128);
  const bool underfill = !act && N % 128 == 0 && N > 96 && tiles128 < 256 && k.opconv_tile != -1;
  // narrow-layer tile variant (diagnostics / A-B): ALCM_OPCONV_TILE=0 default, 1 = twice the rows per tile,
  // 2 = twice the rows and two taps per K step (the split operands need the default tiles' LDS)
  const int v = a.prec != PREC_SPLIT ? k.opconv_tile : 0;
  const bool big = v == 1 || v == 2;
  if (act && N > 96) return fail(p, "opconv: fused activation on N > 96 needs the wide kernel");
  //                                                     BM   BN  WGM WGN TPS
  struct Tile { int BM, BN, WGM, WGN, TPS; } t;
  if (N % 192 == 0 && N % 128 != 0) t = {128, 192, 2, 2, 1};
  else if (N % 128 == 0 && !underfill) t = {128, 128, 2, 2, 1};
  else if (N > 48) t = big ? Tile{256, 96, 4, 1, v} : Tile{128, 96, 2, 2, 1};
  else if (N > 32) t = big ? Tile{512, 48, 4, 1, v} : Tile{256, 48, 4, 1, 1};
  else if (N > 16) t = big ? Tile{512, 32, 4, 1, v} : Tile{256, 32, 4, 1, 1};
  else t = {256, 16, 4, 1, 1};
  // LDS-staged epilogue for narrow layers (one tile spans N); wide layers store straight from the
  // accumulators (measured faster there: the LDS round trip costs more than the coalescing saves)
  const bool vec = N % 4 == 0 && N <= t.BN;
  if (act && !vec) return fail(p, "opconv: fused activation needs N % 4 == 0 and one column tile");
  p->kernel = CK_OPCONV;
  p->BM = t.BM; p->BN = t.BN; p->WGM = t.WGM; p->WGN = t.WGN; p->TPS = t.TPS;
  p->vec = vec; p->act = act;
  // conv1 (no residual) of C = 96 at fp16: the 3-workgroup build (-11..-13 % per launch, scripts/microbench.py
  // tail; the same 128-row build for C = 48 measured +10 % at k11 against its 256-row tiles and is not used)
  p->act3 = act && t.BM == 128 && a.prec == PREC_F16 && !a.res;
  // ACT tiles overlap by 2 * ACT_EPI_HALO rows: each computes BM conv rows and emits BM - 2*HALO
  const int tstride = act ? t.BM - 2 * ACT_EPI_HALO : t.BM;
  p->tiles_per_batch = (a.T + tstride - 1) / tstride;
  p->tiles_n = (N + t.BN - 1) / t.BN;
  p->tiles = p->grid = (int64_t)a.B * p->tiles_per_batch * p->tiles_n;
  // the demangled rocprofv3 name of the instantiation (bench.py joins the two by name); LDS: the split operands
  // double both buffers, so their 192-column tiles take one tap per step
  const int tps = (a.prec == PREC_SPLIT && t.BN >= 192) ? 1 : t.TPS;
  std::snprintf(p->name, sizeof(p->name), "alcm::opconv_kernel<%d, %d, %d, %d, %d, %d, %s, %s, %s>", t.BM, t.BN, t.WGM,
                t.WGN, a.prec, tps, (vec || act) ? "true" : "false", act ? "true" : "false", p->act3 ? "true" : "false");
  return 0;
}

// one-launch sum form (wconv3_kernel<PREC, 3>): three same-length terms with their own planes, weights, taps, biases
// and residuals into one output.  Eligible: the terms' shared B, T, Cp, N and precision (F16 / BF16), dilation 1,
// 3 <= k <= 65, Cp % 64 == 0, N % 192 == 0, full 256-row tiles filling the chip (as wconv3 by shape)
bool sum_one_launch(const alcm_opconv_args* a, int n, int ncu, const Knobs& k) {
  if (n != 3 || k.wconv_sum == 0 || k.wconv <= 0 || k.wconv3 == 0) return false;
  const alcm_opconv_args& a0 = a[0];
  if ((a0.prec != PREC_F16 && a0.prec != PREC_BF16) || a0.Cp % 64 || a0.N % W3_BN) return false;
  // output: fp32 out, or (no accumulate) the operand plane of the value the fp32 route would store
  if (a0.out_plane ? (a0.out || a0.accumulate || (addr(a0.out_plane) & 3)) : !a0.out) return false;
  for (int i = 0; i < n; ++i) {
    const alcm_opconv_args& t = a[i];
    if (t.B != a0.B || t.T != a0.T || t.Cp != a0.Cp || t.N != a0.N || t.prec != a0.prec || t.dil != 1 ||
        t.ksize < 3 || t.ksize - 1 > 64 || 2 * t.pad != t.ksize - 1 || t.out_act || t.out_stride > 0 ||
        t.geglu_plane || (i > 0 && t.out_plane) || t.act_plane || (int64_t)W3_BN * t.kpad * 2 >= (1ll << 31))
      return false;
  }
  const int mt256 = (a0.T + W3_BM - 1) / W3_BM;
  const int64_t nt = (int64_t)a0.B * mt256 * (a0.N / W3_BN);
  const bool full = a0.T * 100 >= mt256 * W3_BM * 85;
  if (!(k.wconv3 > 0 || (full && nt >= ncu))) return false;
  return nt < (1ll << 30) && (int64_t)a0.B * a0.T * a0.Cp < (1ll << 40) && (int64_t)a0.B * a0.T * a0.N < (1ll << 40);
}

}  // namespace

int ksplit_parts(int64_t tiles, int64_t slots, int chunks, double elems, double ws_floats) {
  int ks = 1;
  double best = (double)((tiles + slots - 1) / slots);
  for (int k = 2; k <= 8; ++k) {
    if (chunks % k || chunks / k < 4 || (double)k * elems > ws_floats) continue;
    const double t = (double)((tiles * k + slots - 1) / slots) / k;
    if (t < best * 0.95) {
      best = t;
      ks = k;
    }
  }
  return ks;
}

int conv_plan(const alcm_opconv_args& a, int ncu, const Knobs& k, ConvPlan* p) {
  *p = ConvPlan{};
  p->ksplit = 1;
  if (const char* e = validate_term(a, true)) return fail(p, e);
  const bool act = a.act_plane != nullptr, strided = a.out_stride > 0;
  const double M = (double)a.B * a.T;
  const int npa = a.prec == PREC_SPLIT ? 2 : 1, npb = (a.prec == PREC_SPLIT || a.prec == PREC_F16W2) ? 2 : 1;
  p->flops = 2.0 * M * a.N * (double)a.ksize * a.C;
  p->bytes = M * a.Cp * 2.0 * npa + (double)a.N * a.kpad * 2.0 * npb +
             M * a.N * 4.0 * ((a.out ? 1 : 0) + (a.res ? 1 : 0) + (a.accumulate ? 1 : 0)) +
             (act ? M * round_up(a.N, 32) * 2.0 * npa : 0.0);
  if (a.out_plane) {  // only the wide-layer kernels have the plane-output epilogue
    if (a.res || a.accumulate || a.out_act || act || a.geglu_plane || strided || a.out ||
        (a.prec != PREC_F16 && a.prec != PREC_BF16) || (addr(a.out_plane) & 7) || !plan_wide(a, ncu, k, p))
      return fail(p, "opconv: plane output needs F16/BF16, N % 4 == 0, Cp % 64 == 0, out == NULL "
                     "and no res/accumulate/act/GEGLU/strided output");
    return 0;
  }
  if (a.geglu_plane) {  // only the wide-layer kernel has the GEGLU epilogue
    if (!plan_wide(a, ncu, k, p))
      return fail(p, "opconv: GEGLU plane epilogue needs F16/BF16, N % 128 == 0, Cp % 64 == 0, "
                     "no res/accumulate/act, 4-byte aligned plane");
    return 0;
  }
  if (strided) {  // the two-workgroup wide-layer kernel, or opconv_kernel's LDS-staged epilogue (N <= 96)
    if (plan_wide(a, ncu, k, p)) return 0;
    if (a.N % 4 || a.N > 96)
      return fail(p, "opconv: strided output needs the wide-layer kernel (F16/BF16, N % 192 == 0, "
                     "Cp % 64 == 0, (k-1)*dil <= 64) or N <= 96 with N % 4 == 0");
  } else if ((!act && plan_wide(a, ncu, k, p)) || plan_nconv(a, k, p)) {
    return 0;
  }
  return plan_opconv_kernel(a, k, p);
}

int conv_sum_plan(const alcm_opconv_args* a, int n, int ncu, const Knobs& k, ConvPlan p[3], int* launches) {
  p[0] = ConvPlan{};
  *launches = 0;
  if (!a || n < 1 || n > 3) return fail(p, "opconv_sum: 1 <= n <= 3 terms");
  if (!a[0].out && !a[0].out_plane) return fail(p, "opconv_sum: args[0].out is required");
  for (int i = 0; i < n; ++i)
    if (const char* e = validate_term(a[i], false)) return fail(p, e);
  const bool one = sum_one_launch(a, n, ncu, k);
  if (a[0].out_plane && !one)
    return fail(p, "opconv_sum: a plane output needs the one-launch form (three F16 / BF16 terms, "
                   "dilation 1, Cp % 64 == 0, N % 192 == 0, full 256-row tiles) and no accumulate");
  for (int i = 0; i < n; ++i)
    if (a[i].B != a[0].B || a[i].T != a[0].T || a[i].N != a[0].N || a[i].act_plane || (i > 0 && a[i].out_plane) ||
        a[i].geglu_plane || a[i].out_stride > 0 || a[i].out_act || (a[i].out && a[i].out != a[0].out))
      return fail(p, "opconv_sum: terms need equal B, T, N, same-length fp32 outputs into "
                     "args[0].out, no activation / plane / GEGLU / strided output");
  if (!one) {
    for (int i = 0; i < n; ++i) {
      if (conv_plan(conv_sum_term(a, i), ncu, k, &p[i])) return fail(p, p[i].err);
    }
    *launches = n;
    return 0;
  }
  const alcm_opconv_args& a0 = a[0];
  ConvPlan& q = p[0];
  q.kernel = CK_WCONV3_SUM;
  q.BM = W3_BM; q.BN = W3_BN;
  q.tiles_per_batch = (a0.T + W3_BM - 1) / W3_BM;
  q.tiles_n = a0.N / W3_BN;
  q.tiles = (int64_t)a0.B * q.tiles_per_batch * q.tiles_n;
  q.n_major = 1;
  q.ksplit = 1;
  q.grid = wconv3_grid(q.tiles, ncu, k);
  const double e = (double)a0.B * a0.T;
  q.bytes = e * a0.N * (a0.out_plane ? 2.0 : 4.0 * (a0.accumulate ? 2 : 1));
  for (int i = 0; i < n; ++i) {
    q.flops += 2.0 * e * a0.N * (double)a[i].ksize * a[i].C;
    q.bytes += e * a0.Cp * 2.0 + (double)a0.N * a[i].kpad * 2.0 + (a[i].res ? e * a0.N * 4.0 : 0.0);
  }
  std::snprintf(q.name, sizeof(q.name), "alcm::wconv3_kernel<%d, 3, false>", a0.prec);
  shape_suffix(&q, k, " T%d C%d N%d k%d+%d+%d", a0.T, a0.Cp, a0.N, a[0].ksize, a[1].ksize, a[2].ksize);
  *launches = 1;
  return 0;
}

bool opconv_act_supported(int prec, int N, int Cp_in) {
  if (N % 4 || N <= 0) return false;
  // opconv_kernel ACT tiles (BN <= 96): HBM-bound layers, the fusion saves ~15%.  Wide layers keep conv + standalone
  // Activation1d: a fused epilogue in the two-workgroup wide conv measured -6 % end to end
  return N <= 96;
}

// ------------------------------------------------------------------ the tail convs (alcm_opconv_dense)
bool tconv_supported(const Knobs& k, int prec, int C, int N, int ksize, int dil) {
  if (k.tconv == 0) return false;
  if (prec != PREC_F16 && prec != PREC_F16W2) return false;
  if (C != N || ksize > 11 || (ksize - 1) * dil > 64) return false;
  if (C == 96) return prec == PREC_F16;
  return C == 48 || C == 24;
}

namespace {

// every operand check of alcm_opconv_dense: dense fp16 weights [N][kpad] (K = tap * C + c; lo plane w_lo_off elements
// after hi for F16W2), out / res fp32 [B][T][N], Activation1d of the result into act_plane (or none)
const char* validate_dense(const alcm_opconv_args& a, const Knobs& k) {
  const bool act = a.act_plane != nullptr;
  if (!a.a || !a.w || a.B <= 0 || a.T <= 0) return "opconv_dense: bad arguments";
  if (act && (!a.act_alpha_exp || !a.act_inv_beta || !a.act_up_filter || !a.act_down_filter || a.N % 2))
    return "opconv_dense: activation parameters";
  if (!tconv_supported(k, a.prec, a.C, a.N, a.ksize, a.dil)) return "tconv: unsupported shape";
  if (a.C <= 0 || a.Cp < a.C || a.ksize < 1 || a.dil < 1) return "tconv: bad geometry";
  if (a.kpad != round_up(a.ksize * a.C, 32)) return "tconv: dense weight layout";
  if (2 * a.pad != (a.ksize - 1) * a.dil || a.out_stride > 0 || a.out_act || a.geglu_plane)
    return "tconv: same-length convs only";
  // (the fp16 weight plane the kernels read lies 2 * w_lo_off elements behind w: aligned where w and w_lo_off are)
  if ((addr(a.a) & 15) || (addr(a.w) & 15) || (a.w_lo_off % 8) || (a.Cp % 8) || (a.res && (addr(a.res) & 15)) ||
      (a.out && (addr(a.out) & 15)))
    return "tconv: alignment";
  if (act && (a.accumulate || (a.out && !a.res))) return "tconv: epilogue combination";
  // tiles recompute ACT_EPI_HALO rows on each side: a neighbour's state rows must still hold the residual
  if (act && a.out && (const void*)a.out == (const void*)a.res) return "tconv: fused activation: out aliases res";
  if (act && (addr(a.act_plane) & 3)) return "tconv: act_plane alignment";
  if (a.out_plane) return "tconv: no plane output";
  return nullptr;
}

}  // namespace

int dense_conv_plan(const alcm_opconv_args& a, int ncu, const Knobs& k, ConvPlan* p) {
  *p = ConvPlan{};
  p->ksplit = 1;
  if (const char* e = validate_dense(a, k)) return fail(p, e);
  const bool act = a.act_plane != nullptr;
  const int C = a.C, ks = a.ksize, npb = a.prec == PREC_F16W2 ? 2 : 1;
  // ALCM_TCONV: 1 by shape, 2 streamed weights (two workgroups per CU) wherever the shape allows, 3 resident weights.
  // Measured per launch (scripts/microbench.py tconv): streamed wins at C = 96 and C = 24, resident at C = 48
  const int tk = k.tconv;
  const bool streamed = tk == 2 || (tk != 3 && tk != 4 && C != 48);
  // ALCM_TCONV=4 (C = 48): column halves (NS = 24, the B fragments of columns 24..31 read one zero row) on 128-row
  // tiles, so the resident weights (k11: 54 KB) and the window leave room for two workgroups per CU
  const bool half48 = !streamed && C == 48 && (tk == 4 || tk == 5);
  const int occ48 = (tk == 5 && ks <= 3) ? 3 : 2;  // ALCM_TCONV=5: k = 3 at three workgroups per CU
  // resident C = 48 at F16W2: the LDS weight region sized by the taps (k <= 7 leaves room for the window apart from
  // the staged tile); every other instantiation reserves 11 taps
  const int kmax48 = npb == 2 ? (ks <= 3 ? 3 : (ks <= 7 ? 7 : 11)) : 11;
  int wgs = 0;  // persistent grids: workgroups per CU; 0 = one workgroup per tile
  if (streamed) {
    p->kernel = CK_TCONV2;
    p->block = 256;
    p->NS = C;
    p->BM = C == 96 ? 192 : 256;
    if (C == 96) {
      // persistent, two workgroups per CU, the second half delayed by 2 sleeps (scripts/microbench.py tconv, one box:
      // k11 0.547 -> 0.491 ms, k3 0.300 -> 0.301, conv2 + residual 0.732 -> 0.695)
      p->R = 11; p->OCC = 2; p->STG = 2;
      wgs = 2;
    } else if (C == 48) {
      p->R = 24; p->OCC = 2;
    } else if (npb == 2) {
      // C = 24 one workgroup per tile (persistent measured +5..+17 %), four workgroups per CU (6-row Activation1d runs
      // and the residual loaded in the epilogue keep it at 128 VGPRs): conv2 + residual + Activation1d 0.61 -> 0.51 ms
      // (k3), 0.70 -> 0.55 (k11), conv1 k3 0.39 -> 0.37, end to end -0.5 ms/step
      p->R = 6; p->OCC = 4;
    } else {
      // (other policies; a W1 twin of the W2 instantiation's template arguments above made the compiler spill 84 B in
      // the W2 kernel, 12 without)
      p->R = 12; p->OCC = 2;
    }
  } else {
    p->kernel = CK_TCONV;
    if (C == 96) {  // two column halves: the 96 x 1056 weight matrix does not fit one CU's LDS
      p->NS = 48; p->BM = 192; p->R = 11; p->KMAX = 11; p->OCC = 1;
    } else if (half48) {
      // (F16 has the one 11-tap, two-per-CU instantiation; at ALCM_TCONV=5, k = 3 its grid is still three per CU)
      p->NS = 24; p->BM = 128; p->R = 7; p->KMAX = kmax48; p->OCC = npb == 2 ? occ48 : 2;
    } else if (C == 48) {
      p->NS = 48; p->BM = 256; p->R = 12; p->KMAX = kmax48; p->OCC = 1;
    } else {
      p->NS = 24; p->BM = 256; p->R = 6; p->KMAX = 11; p->OCC = 1;
    }
    p->block = p->BM * 2 + 64;
    wgs = half48 ? occ48 : (C == 24 ? 2 : 1);  // C = 24 fits two per CU
  }
  p->C = C; p->NPB = npb; p->BN = p->NS;
  p->act = act;
  const int slots = a.kpad / 8;
  p->wslots = slots % 2 ? slots : slots + 1;
  p->ncg = p->tiles_n = a.N / p->NS;
  // tiles overlap by 2 * ACT_EPI_HALO rows: each computes BM conv rows and emits BM - 2 * HALO
  p->tiles_per_batch = (a.T + (p->BM - 2 * ACT_EPI_HALO) - 1) / (p->BM - 2 * ACT_EPI_HALO);
  p->tiles = (int64_t)a.B * p->tiles_per_batch * p->ncg;
  if (p->tiles >= (1ll << 30)) return fail(p, "tconv: problem too large");
  p->grid = wgs ? std::min<int64_t>(p->tiles, (int64_t)ncu * wgs) : p->tiles;
  // resident: a multiple of ncg workgroups so a workgroup's column group (blockIdx % ncg) is the same for every tile
  // it takes (tile % ncg == blockIdx % ncg)
  if (!streamed) p->grid = std::max<int64_t>(p->ncg, p->grid / p->ncg * p->ncg);
  const bool res = a.res != nullptr, out = a.out != nullptr;
  if (act && !res && !out) p->epi = TE_CONV1;
  else if (act && res && out) p->epi = TE_CONV2;
  else if (!act && res && out) p->epi = TE_LAST;
  else return fail(p, "tconv: unsupported epilogue combination");
  const double M = (double)a.B * a.T;
  p->flops = 2.0 * M * a.N * (double)ks * C;
  p->bytes = M * C * 2.0 + (double)a.N * a.kpad * 2.0 * npb +
             M * a.N * 4.0 * ((out ? 1 : 0) + (res ? 1 : 0) + (a.accumulate ? 1 : 0)) + (act ? M * a.N * 2.0 : 0.0);
  // the historical profile row (bench.py and the recorded profiles join by it); the template-id is p->inst
  std::snprintf(p->name, sizeof(p->name), "alcm::tconv%s_kernel<C%d, W%d, BM%d, %s%s%s>", streamed ? "2" : "", C, npb,
                p->BM, act ? "act" : "", res ? "+res" : "", p->epi == TE_LAST ? "+acc" : "");
  shape_suffix(p, k, " T%d k%d", a.T, ks, 0);
  static const char* const kEpi[] = {"true, false, false, false", "true, true, true, false",
                                     "false, true, false, true"};  // ACT, RES, OUTW, ACC
  if (streamed)
    std::snprintf(p->inst, sizeof(p->inst), "tconv2_kernel<%d, %d, %d, %d, %d, %s, %d, %d>", C, p->NS, npb, p->BM, p->R,
                  kEpi[p->epi], p->OCC, p->STG);
  else
    std::snprintf(p->inst, sizeof(p->inst), "tconv_kernel<%d, %d, %d, %d, %d, %d, %d, %s>", C, p->NS, npb, p->BM, p->R,
                  p->KMAX, p->OCC, kEpi[p->epi]);
  return 0;
}

}  // namespace alcm
