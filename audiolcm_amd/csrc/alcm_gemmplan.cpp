// The fp32-operand GEMM planner (alcm_gemmplan.h): one validator and one kernel choice for alcm_gemm.  Order of
// preference: conv_kernel (k > 1 on one staged window), gemm_skinny_kernel (few rows, k = 1), gemm_kernel's tile ladder.
#include "alcm_gemmplan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace alcm {

namespace {

constexpr int PREC_BF16 = ALCM_PREC_BF16, PREC_SPLIT = ALCM_PREC_SPLIT, PREC_F16 = ALCM_PREC_F16;
constexpr int ACT_NONE = 0, ACT_SILU = 1;  // the prologue's activation codes (AlcmAct, alcm_common.h)

int fail(GemmPlan* p, const char* msg) {
  p->err = msg;
  return ALCM_E_INVALID;
}

// whether an ACT operand's rows can be read as 16-byte vectors of channels
inline bool act_vec_ok(const alcm_operand& o) {
  const bool al = (((uintptr_t)o.ptr) & 15) == 0;
  return al && o.sc == 1 && o.C_in == o.Cpad && o.Cpad % 8 == 0 && o.st % 4 == 0 && o.sb % 4 == 0 &&
         o.zs1 % 4 == 0 && o.zs2 % 4 == 0;
}

// the checks of an ACT operand, A or B (which: 0 / 1)
const char* validate_act(const alcm_operand& o, int which) {
  const int up = o.up ? o.up : 1;
  if (!o.ptr || o.Cpad <= 0 || o.Cpad % 8 || o.C_in > o.Cpad || o.ksize <= 0 || o.T_in <= 0 || (up != 1 && up != 2) ||
      o.rows_per_batch <= 0)
    return which ? "B: bad ACT operand geometry" : "A: bad ACT operand geometry";
  if (o.pro_act != ACT_NONE && o.pro_act != ACT_SILU)
    return which ? "B: prologue activation must be NONE or SILU" : "A: prologue activation must be NONE or SILU";
  if ((o.pro_scale == nullptr) != (o.pro_shift == nullptr) || (o.pro_mean == nullptr) != (o.pro_rstd == nullptr))
    return which ? "B: prologue scale/shift and mean/rstd must come in pairs"
                 : "A: prologue scale/shift and mean/rstd must come in pairs";
  return nullptr;
}

// every operand check of alcm_gemm but the one that depends on the kernel choice (an ACT / ACT_T B operand needs a
// vectorisable A: gemm_plan)
const char* validate(const alcm_gemm_args& g) {
  if (g.Kpad <= 0 || g.Kpad % BK) return "Kpad must be a positive multiple of 32";
  if (g.a.kind != ALCM_OPND_ACT) return "A operand must be ACT";
  if (!g.out) return "null output";
  if (g.geglu && (g.N % 2)) return "geglu needs even N";
  if (const char* e = validate_act(g.a, 0)) return e;
  if (g.a.ksize * g.a.Cpad > g.Kpad) return "Kpad smaller than ksize*Cpad of A";
  if (g.b.kind == ALCM_OPND_WEIGHT) {
    if (!g.b.ptr || g.b.rows < g.N) return "weight operand rows < N";
    if ((((uintptr_t)g.b.ptr) & 15) || (g.b.w_lo_off % 8)) return "weight alignment";
  } else if (g.b.kind == ALCM_OPND_ACT) {
    if (const char* e = validate_act(g.b, 1)) return e;
    if (!act_vec_ok(g.b) || g.b.ksize != 1 || g.b.pro_scale || g.b.pro_mean)
      return "B ACT operand must be channel-contiguous, 16B aligned, k=1, no prologue";
    if (g.b.ksize * g.b.Cpad > g.Kpad) return "Kpad smaller than B K";
  } else if (g.b.kind == ALCM_OPND_ACT_T) {
    if (!g.b.ptr || g.b.rows < g.N) return "ACT_T operand rows < N";
  } else {
    return "unknown B operand kind";
  }
  if (g.prec < PREC_BF16 || g.prec > PREC_F16) return "prec must be 0 (bf16), 1 (split) or 2 (f16)";
  return nullptr;
}

// algorithmic work of the launch: 2*M*N*K_real MACs; unique A rows, B operand, output (+ residual / accumulate)
void cost(const alcm_gemm_args& g, int bkind, GemmPlan* p) {
  const double Kr = (double)g.a.ksize * g.a.C_in;
  const double nb = (double)(g.batch > 0 ? g.batch : 1);
  const double a_rows = (double)g.a.T_in * ((double)g.M / std::max(1, g.a.rows_per_batch));
  double bbytes;
  if (bkind == BK_W) bbytes = (double)g.N * g.Kpad * 2.0 * (g.prec == PREC_SPLIT ? 2 : 1);
  else if (bkind == BK_ACT) bbytes = nb * (double)g.b.T_in * g.b.C_in * 4.0;
  else bbytes = nb * (double)g.b.rows * g.b.T_in * 4.0;
  const double nout = g.geglu ? g.N / 2 : g.N;
  const double obytes = nb * (double)g.M * nout * 4.0 * (1 + (g.res ? 1 : 0) + (g.accumulate ? 1 : 0));
  p->flops = 2.0 * nb * (double)g.M * g.N * Kr;
  p->bytes = nb * a_rows * g.a.C_in * 4.0 + bbytes + obytes;
}

// the profile row: the demangled rocprofv3 name of the instantiation; under ALCM_PROF_SHAPES a suffix splits the
// statistics per problem shape
void shape_suffix(GemmPlan* p, const Knobs& k, const char* fmt, int v0, int v1, int v2, int v3 = 0, int v4 = 0,
                  int v5 = 0) {
  if (!k.prof_shapes) return;
  const size_t n = std::strlen(p->name);
  std::snprintf(p->name + n, sizeof(p->name) - n, fmt, v0, v1, v2, v3, v4, v5);
}

void tile(GemmPlan* p, int BM, int BN, int WM, int WN) {
  p->BM = BM; p->BN = BN; p->WM = WM; p->WN = WN;
}

}  // namespace

int gemm_plan(const alcm_gemm_args& g, const Knobs& k, bool want_profile, GemmPlan* p) {
  *p = GemmPlan{};
  if (g.M <= 0 || g.N <= 0) return 0;  // GF_NONE
  if (const char* e = validate(g)) return fail(p, e);
  const int N = g.N, batch = g.batch > 0 ? g.batch : 1, up = g.a.up ? g.a.up : 1;
  const int bkind = g.b.kind == ALCM_OPND_WEIGHT ? BK_W : (g.b.kind == ALCM_OPND_ACT ? BK_ACT : BK_ACTT);
  const bool avec = act_vec_ok(g.a);
  p->bkind = bkind; p->prec = g.prec; p->avec = avec;
  if (want_profile) cost(g, bkind, p);

  // conv_kernel: k > 1 taps as shifted views of one input window staged per 32-channel chunk, so the A loads, the
  // fp32 -> operand conversions and the A LDS writes happen once instead of k times (k = 3..11 on the path).  Eligible:
  // whole clips of channel-contiguous, unpadded rows (tiles never straddle a clip), Cpad % 32 == 0, (k-1) d <= HALO_MAX
  const bool window_conv = bkind == BK_W && avec && batch == 1 && g.a.ksize > 1 && g.a.Cpad % 32 == 0 &&
                           g.a.C_in == g.a.Cpad && (g.a.ksize - 1) * g.a.dil <= HALO_MAX &&
                           g.out_rows_per_batch == g.a.rows_per_batch && g.M % g.a.rows_per_batch == 0 &&
                           !g.disable_window;
  if (window_conv) {
    p->family = GF_WINDOW_CONV;
    p->nbatch = g.M / g.a.rows_per_batch;
    p->T_out = g.a.rows_per_batch;
    // 64-wide N tiles when 128-wide tiles would waste a third of the MFMA work (N = 192, 320, ...)
    const bool narrow = g.tile_n == 64 || (g.tile_n == 0 && (N <= 64 || (N % 128 != 0 && N % 64 == 0)));
    if (narrow) tile(p, 128, 64, 4, 1);
    else tile(p, 128, 128, 2, 2);
    p->pro = g.a.pro_scale || g.a.pro_mean || g.a.pro_act;
    p->tpb = (p->T_out + p->BM - 1) / p->BM;
    p->gx = p->nbatch * p->tpb; p->gy = (N + p->BN - 1) / p->BN; p->gz = 1;
    if (want_profile) {
      std::snprintf(p->name, sizeof(p->name), "alcm::conv_kernel<%d, %d, %d, %d, %d, %s>", p->BM, p->BN, p->WM, p->WN,
                    g.prec, p->pro ? "true" : "false");
      shape_suffix(p, k, " T%d N%d K%d k%d up%d x%d", p->T_out, N, g.Kpad, g.a.ksize, up, p->nbatch);
    }
  } else if (bkind == BK_W && batch == 1 && g.M <= SK_MAXM && g.a.ksize == 1 && g.a.pad == 0 && up != 2 &&
             !g.a.pro_mean && !g.a.pro_scale && !g.a.pro_act && !g.geglu && g.Kpad <= SK_KMAX && g.Kpad % 8 == 0 &&
             g.a.sc == 1 && g.a.C_in % 4 == 0 && g.a.st % 4 == 0 && g.a.sb % 4 == 0 &&
             (((uintptr_t)g.a.ptr) & 15) == 0 && k.gemm_skinny) {
    // gemm_skinny_kernel: the DiT embedder MLPs' M = B rows (Linear -> SiLU -> Linear).  On the MFMA tiles a 32-row
    // problem is 1-5 workgroups walking K serially, ~45 us a launch; here 32 columns x 8 K slices per workgroup on fixed
    // 32-row blocks: 6 launches 0.28 -> 0.16 ms/step.  Eligibility depends on K (the LDS block, SK_KMAX) and the layer,
    // never on M below SK_MAXM, so a row's arithmetic does not depend on how a batch is split (ALCM_GEMM_SKINNY=0: the
    // MFMA tiles)
    p->family = GF_SKINNY;
    p->BM = SK_M; p->BN = SK_N;
    p->gx = (N + SK_N - 1) / SK_N; p->gy = (g.M + SK_M - 1) / SK_M; p->gz = 1;
    if (want_profile) {
      std::snprintf(p->name, sizeof(p->name), "alcm::gemm_skinny_kernel<%d>", g.prec);
      shape_suffix(p, k, " M%d N%d K%d", g.M, N, g.Kpad);
    }
  } else {
    // an ACT / ACT_T B operand (the attention products): gemm_kernel is built for them with vector A loads only
    if (bkind != BK_W && !avec) return fail(p, "attention GEMM A operand must be vectorisable");
    p->family = GF_GEMM;
    if (bkind == BK_W && N <= 32 && (int64_t)((g.M + 255) / 256) * batch < 128 && k.gemm_skinny) {
      // N <= 32 on fewer than 128 tiles of 256 rows: 64-row tiles, 4x the workgroups.  The DiT final layer (B T = 9984
      // rows x N = 20): 39 -> 156 workgroups, 0.20 -> 0.08 ms/step; the same K order per output, so bit-identical
      // (ALCM_GEMM_SKINNY=0: the 256-row tiles)
      tile(p, 64, 32, 4, 1);
    } else if (bkind == BK_W && N <= 32) {
      tile(p, 256, 32, 4, 1);
    } else if (N <= 64) {
      tile(p, 256, 64, 4, 1);  // one column tile of four waves stacked on rows
    } else {
      tile(p, 128, 128, 2, 2);
    }
    p->gx = (g.M + p->BM - 1) / p->BM; p->gy = (N + p->BN - 1) / p->BN; p->gz = batch;
    if (want_profile) {
      std::snprintf(p->name, sizeof(p->name), "alcm::gemm_kernel<%d, %d, %d, %d, %s, %d, %d>", p->BM, p->BN, p->WM,
                    p->WN, avec ? "true" : "false", bkind, g.prec);
      shape_suffix(p, k, " M%d N%d K%d x%d", g.M, N, g.Kpad, batch);
    }
  }
  return 0;
}

}  // namespace alcm
