// dfe_tgt.hip -- the target-side deep feature embedding, collapsed form (the default of
// dvcp_dfe_tgt, and dvcp_dfe_tgt_f16); dfe_mfma.h lists the units.
//
// fc1, fc2 and fc3 have no nonlinearity between them (Q14, deep_feat_embedding.py:48-50), so
// fc3(fc2(fc1 x)) = E x + e with E = W3 W2 W1 (32 x 35) and e = W3 (W2 b1 + b2) + b3.  Each
// workgroup forms E and e in fp64 from the three layers (a 72 kflop prologue) and rounds them once
// to fp32; a candidate then costs one 35-deep product instead of three layers.
// The result differs from the layer-by-layer fp32 chain only by rounding (two fewer fp32
// roundings of intermediates, one of E); tests hold it to the same 1e-5 bound.
//   H = X . E^T:  A = X (lane: row j, k-half), B = E^T fragment (lane: output channel, k-half)
//   -> output channel on lanes, rows in registers, max over rows = registers + one lane swap.
// The xyz columns take two fp32 MFMA k-steps ((x|y), (z|0)) and the 32 feature columns two 16-deep
// bf16 k-steps of the fp32-accurate three-way split (lane half h's features 16h + 8t .. + 7 in
// k-step t): 2 x 64 + 12 x 32 = 512 MFMA cycles per candidate instead of the 19 x 64 = 1216 of 19
// fp32 k-steps.
// dist_sum: 32 fp32 distances summed in fp64 are exact whenever they span less than 2^24 (24-bit
// mantissas, 5 bits of carry, 53-bit accumulator), so a butterfly sum equals the reference's
// ordered sum; w_j = dist_j / dist_sum in fp64 is then bit-identical.
// (DESIGN.md section 4 has the measurements behind the choices fixed here: the grid size, the
// waves per SIMD, the w rows formed two steps ahead and two at a time, the scalar candidate loads,
// and the alternatives that were measured and not kept.)
#include "dfe_mfma.h"

#include <type_traits>

namespace dvcp {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// x = x0 + x1 + x2 exactly in three bf16 pieces; a.b from the six significant piece products
// (the fp32-accurate split of sa_mfma_common.h, whose header gives the error bound)
struct DfeSplit3 {
  bf16x8 p0, p1, p2;
};
__device__ __forceinline__ DfeSplit3 dfe_split3(const float (&x)[8]) {
  DfeSplit3 s;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 b0 = static_cast<__bf16>(x[j]);
    const float r1 = x[j] - static_cast<float>(b0);
    const __bf16 b1 = static_cast<__bf16>(r1);
    s.p0[j] = b0;
    s.p1[j] = b1;
    s.p2[j] = static_cast<__bf16>(r1 - static_cast<float>(b1));
  }
  return s;
}
__device__ __forceinline__ f32x16 dfe_mfma_split3(const DfeSplit3& a, const bf16x8& b0, const bf16x8& b1,
                                                 const bf16x8& b2, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p2, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p1, b1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p0, b2, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p1, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p0, b1, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p0, b0, acc, 0, 0, 0);
}

constexpr int kDfe1Waves = 4;
// workgroups (a multiple of 8), every wave resident from the start (one fp64 prologue per
// workgroup, no tail of late workgroups): two workgroups per CU (two waves per SIMD) keep the
// gathers and the matrix cores as busy as three, and leave the CU room to other kernels' waves
constexpr int kDfeGrid = 512;

// v + (v moved by the DPP pattern CTRL), fp64 (the two halves moved separately).  Every pattern
// used (quad permutes, row rotations) reads a lane of the same row for every lane, so the moves
// need no old value (mov_dpp: no zeroed destination register per move)
template <int CTRL>
__device__ __forceinline__ double dpp_add_f64(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
  return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

struct Dfe1Lds {
  double p[32][35];      // W2 . W1 (fp64), prologue only
  double pb[32];         // W2 . b1 + b2
  float ex[2][64];          // E's xyz columns as fp32 B fragments: k-steps (x|y), (z|0)
  bf16x8 es[2][3][64];      // E's feature columns as bf16 pieces: [k-step][piece][lane]
  float eb[32];          // e
  float w[kDfe1Waves][4][32];  // per-wave w rows of consecutive candidates (fp64 quotient rounded to fp32)
};

// FT: the feature table's element type -- float, or _Float16 (the C5 "fp16 features" storage:
// half the gathered bytes; each row is widened to fp32 before the weighting, which then runs in
// fp32 exactly as for a float table holding the same values).
// P4: the target points are (x, y, z, pad) float4 rows (PointsView::rows4, dvcp_points_pack4,
// known at launch): one 16-byte gather per neighbour instead of three 4-byte loads from three
// lines of the (B, 3, M) layout, with no per-candidate layout branch.
// Compiled for three waves per SIMD (136 VGPRs, no spills; four: 128 VGPRs and 48 B of spills).
template <typename T, typename FT = float, bool P4 = false>
__global__ __launch_bounds__(kDfe1Waves * kWave) __attribute__((amdgpu_waves_per_eu(3))) void dfe_tgt_mfma1_kernel(
    PointsView<T> ref, const FT* __restrict__ feat, int M, const float* __restrict__ cand,
    const float* __restrict__ dist, const int32_t* __restrict__ idx, int Q, int B, const float* __restrict__ params,
    float* __restrict__ out, int xcd) {
  __shared__ Dfe1Lds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const float* W1 = params;
  const float* pb1 = W1 + 32 * 35;
  const float* W2 = pb1 + 32;
  const float* pb2 = W2 + 32 * 32;
  const float* W3 = pb2 + 32;
  const float* pb3 = W3 + 32 * 32;
  // prologue: P = W2 W1, pb = W2 b1 + b2 (fp64)
  for (int i = tid; i < 32 * 36; i += blockDim.x) {
    const int o = i / 36, c = i % 36;
    double acc = 0.0;
    if (c < 35) {
      for (int a = 0; a < 32; ++a) acc = __fma_rn(static_cast<double>(W2[o * 32 + a]), static_cast<double>(W1[a * 35 + c]), acc);
      L.p[o][c] = acc;
    } else {
      for (int a = 0; a < 32; ++a) acc = __fma_rn(static_cast<double>(W2[o * 32 + a]), static_cast<double>(pb1[a]), acc);
      L.pb[o] = acc + static_cast<double>(pb2[o]);
    }
  }
  __syncthreads();
  // E = W3 P in fragment order, e = W3 pb + b3
  auto e_entry = [&](int o, int ch) {
    double acc = 0.0;
    for (int a = 0; a < 32; ++a) acc = __fma_rn(static_cast<double>(W3[o * 32 + a]), L.p[a][ch], acc);
    return static_cast<float>(acc);
  };
  for (int i = tid; i < 2 * 64; i += blockDim.x) {
    const int l = i % 64, s = i / 64, hh = l >> 5, o = l & 31;
    const int ch = s == 0 ? hh : (hh == 0 ? 2 : -1);
    L.ex[s][l] = ch < 0 ? 0.0f : e_entry(o, ch);
  }
  for (int i = tid; i < 2 * 64; i += blockDim.x) {
    const int l = i % 64, t = i / 64, hh = l >> 5, o = l & 31;
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = e_entry(o, 3 + 16 * hh + 8 * t + j);
    const DfeSplit3 ws = dfe_split3(w);
    L.es[t][0][l] = ws.p0;
    L.es[t][1][l] = ws.p1;
    L.es[t][2][l] = ws.p2;
  }
  for (int o = tid; o < 32; o += blockDim.x) {
    double acc = 0.0;
    for (int a = 0; a < 32; ++a) acc = __fma_rn(static_cast<double>(W3[o * 32 + a]), L.pb[a], acc);
    L.eb[o] = static_cast<float>(acc + static_cast<double>(pb3[o]));
  }
  __syncthreads();
  const float eb = L.eb[r32];

  // Software pipeline over this wave's candidates g0, g0 + stride, ...: the kNN row (dist, idx)
  // is loaded ahead of the gathered point/feature row, and that ahead of its use, so the
  // dependent idx -> gather latency overlaps the MFMAs of the candidate in hand.  Register
  // sets alternate, so no loaded register is ever copied (a copy would wait for its load).
  // Loads are unconditional (indices clamped to the last candidate) and a loaded index is only
  // clamped in the iteration that gathers with it.  Candidate indices are wave-uniform int32
  // (B * Q < 2^31 is checked by the launcher).
  // Candidate order.  xcd == 0: one index space over all B*Q candidates.  xcd != 0 (B >= 8, grid a
  // multiple of 8): workgroups are dispatched to the 8 XCDs round robin (blockIdx % 8), so the
  // workgroups of XCD x take the candidates of pairs x, x+8, ...; each pair's gathered feature
  // table then lives in one XCD's L2 instead of being fetched into all eight.
  int total, stride, g, xo = 0, P = 1;
  if (xcd) {
    xo = static_cast<int>(blockIdx.x) & 7;
    P = 8;
    total = ((B - xo + 7) / 8) * Q;
    stride = static_cast<int>(gridDim.x >> 3) * kDfe1Waves;
    g = static_cast<int>(blockIdx.x >> 3) * kDfe1Waves + __builtin_amdgcn_readfirstlane(wave);
  } else {
    total = B * Q;
    stride = static_cast<int>(gridDim.x) * kDfe1Waves;
    g = static_cast<int>(blockIdx.x) * kDfe1Waves + __builtin_amdgcn_readfirstlane(wave);
  }
  if (g >= total) return;
  // Local candidate index li = pl * Q + q -> pair b = xo + P * pl and global candidate b * Q + q,
  // tracked incrementally per pipeline slot (wave-uniform, no integer division per candidate);
  // indices past the end clamp to the last candidate (loads stay in bounds, results unused).
  // A tracker holds its pair bb and global candidate gc = bb Q + q as well, advanced by constant
  // steps, so a use is one select against the last candidate instead of a multiply-add chain.
  struct Cand {
    int li, q, bb, gc;
  };
  auto cand_at = [&](int li) {
    Cand c;
    c.li = li;
    const int pl = li / Q;  // once per slot at the start
    c.q = li - pl * Q;
    c.bb = xo + P * pl;
    c.gc = c.bb * Q + c.q;
    return c;
  };
  const int st_pl = stride / Q, st_q = stride - st_pl * Q;
  const int st_bb = P * st_pl, st_gc = P * st_pl * Q + st_q, wrap_gc = (P - 1) * Q;
  auto advance = [&](Cand& c) {  // branch-free (scalar selects): li += stride
    c.li += stride;
    c.q += st_q;
    c.bb += st_bb;
    c.gc += st_gc;
    const bool wrap = c.q >= Q;
    c.q = wrap ? c.q - Q : c.q;
    c.bb = wrap ? c.bb + P : c.bb;
    c.gc = wrap ? c.gc + wrap_gc : c.gc;
  };
  const Cand last = cand_at(total - 1);
  auto pair_of = [&](const Cand& c) { return c.li < total ? c.bb : last.bb; };
  auto glob_of = [&](const Cand& c) { return c.li < total ? c.gc : last.gc; };
  auto load_row = [&](const Cand& c, float& dj, int& n) {
    const int gc = glob_of(c);
    dj = dist[static_cast<int64_t>(gc) * 32 + r32];
    n = idx[static_cast<int64_t>(gc) * 32 + r32];
  };
  struct Gathered {
    float4 f[4];
    uint4 hf[2];  // fp16 table: the row's 16 halves of this lane half, widened in prep
    T px, py, pz;
    float cx, cy, cz;
  };
  auto gather = [&](const Cand& c, int nraw, Gathered& G) {
    const int bb = pair_of(c);
    const int gc = glob_of(c);
    const int n = nraw < 0 ? 0 : (nraw >= M ? M - 1 : nraw);
    if constexpr (sizeof(FT) == 4) {
      const float4* fr = reinterpret_cast<const float4*>(feat + (static_cast<int64_t>(bb) * M + n) * 32 + 16 * h);
#pragma unroll
      for (int v = 0; v < 4; ++v) G.f[v] = fr[v];
    } else {
      const uint4* fr = reinterpret_cast<const uint4*>(feat + (static_cast<int64_t>(bb) * M + n) * 32 + 16 * h);
      G.hf[0] = fr[0];
      G.hf[1] = fr[1];
    }
    if constexpr (P4) {
      const float4 q = *reinterpret_cast<const float4*>(ref.p + bb * ref.sb + 4 * static_cast<int64_t>(n));
      G.px = q.x;
      G.py = q.y;
      G.pz = q.z;
    } else {
      G.px = ref.at(bb, 0, n);
      G.py = ref.at(bb, 1, n);
      G.pz = ref.at(bb, 2, n);
    }
    // the candidate's coordinates as scalar loads (its index is wave-uniform)
    const float* cq = cand + static_cast<int64_t>(__builtin_amdgcn_readfirstlane(gc)) * 3;
    G.cx = cq[0];
    G.cy = cq[1];
    G.cz = cq[2];
  };
  // get_cat_feat_tgt.py:57-58: the w rows of two candidates at once, into the wave's LDS rows bufa
  // and bufb (four rows: a candidate's row is written while earlier ones may still be read).  Lane
  // half 0 forms candidate A's row (dja), half 1 candidate B's (djb), so the fp64 sum, division and
  // DPP moves run once for two candidates.  The sum of the 32 distances: quad and row rotations by
  // DPP (no LDS round trips; the patterns stay inside 16-lane rows, so the halves' sums do not mix:
  // rows 0-1 are A's 32 distances, rows 2-3 B's), then each half's two 16-lane row totals read
  // back and added.  w = dist / dist_sum is formed in fp64 like the reference and rounded once to
  // fp32; the feature product is then one fp32 multiply (the reference rounds the fp64 product to
  // fp32 at the DFE input: the two differ by at most one fp32 ulp of the input).
  auto weights2 = [&](float dja, float djb, int bufa, int bufb) {
    const float dj = h ? djb : dja;
    double v = static_cast<double>(dj);
    v = dpp_add_f64<0xB1>(v);   // quad_perm [1,0,3,2]
    v = dpp_add_f64<0x4E>(v);   // quad_perm [2,3,0,1]
    v = dpp_add_f64<0x124>(v);  // row_ror:4
    v = dpp_add_f64<0x128>(v);  // row_ror:8
    const double sa = readlane_f64(v, 15) + readlane_f64(v, 31);
    const double sb = readlane_f64(v, 47) + readlane_f64(v, 63);
    L.w[wave][h ? bufb : bufa][r32] = static_cast<float>(static_cast<double>(dj) / (h ? sb : sa));
  };
  // A operands of a candidate: the xyz k-steps ((dx|dy), (dz|0)) and the 32 weighted features as
  // split-3 bf16 pieces (lane half h: features 16h .. 16h + 15, k-step t: 16h + 8t ..)
  struct Prepared {
    float x0, x1;
    DfeSplit3 s[2];
  };
  auto prep = [&](const Gathered& G, int buf, Prepared& X) {
    // candidates_grouped_local = tgt_pts_picked - candidate (point dtype, then .float()); half 1: 0
    const float ddx = static_cast<float>(G.px - static_cast<T>(G.cx));
    const float ddy = static_cast<float>(G.py - static_cast<T>(G.cy));
    const float ddz = static_cast<float>(G.pz - static_cast<T>(G.cz));
    X.x0 = h == 0 ? ddx : ddy;
    X.x1 = h == 0 ? ddz : 0.0f;
    const float4* wr = reinterpret_cast<const float4*>(&L.w[wave][buf][16 * h]);
    float4 fv[4];
    if constexpr (sizeof(FT) == 4) {
#pragma unroll
      for (int v = 0; v < 4; ++v) fv[v] = G.f[v];
    } else {
      const uint32_t* hw = reinterpret_cast<const uint32_t*>(G.hf);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint32_t lo = hw[2 * v], hi = hw[2 * v + 1];
        fv[v].x = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(lo & 0xFFFFu)));
        fv[v].y = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(lo >> 16)));
        fv[v].z = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(hi & 0xFFFFu)));
        fv[v].w = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(hi >> 16)));
      }
    }
    float x[16];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float4 w4 = wr[v];
      x[4 * v] = fv[v].x * w4.x;
      x[4 * v + 1] = fv[v].y * w4.y;
      x[4 * v + 2] = fv[v].z * w4.z;
      x[4 * v + 3] = fv[v].w * w4.w;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float f8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f8[j] = x[8 * t + j];
      X.s[t] = dfe_split3(f8);
    }
  };
  // H = X E^T on the matrix cores; zero-started accumulators, e added once to the row maximum:
  // max_j fl(h_j + e) = fl(max_j h_j + e) (rounding is monotone)
  auto mfma = [&](const Prepared& X) {
    int zo = 0;  // opaque zero: E fragments are re-read from LDS per candidate, not hoisted
    asm volatile("" : "+v"(zo));
    f32x16 a;
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.0f;
    a = __builtin_amdgcn_mfma_f32_32x32x2f32(X.x0, L.ex[0][lane + zo], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_32x32x2f32(X.x1, L.ex[1][lane + zo], a, 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 2; ++t)
      a = dfe_mfma_split3(X.s[t], L.es[t][0][lane + zo], L.es[t][1][lane + zo], L.es[t][2][lane + zo], a);
    return a;
  };
  auto finish = [&](const Cand& cg, const f32x16& a) {
    float m = a[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) m = fmaxf(m, a[r]);
    // the other lane half's rows: v_permlane32_swap (lanes 0..31 receive lanes 32..63; only they
    // store) instead of an LDS-crossbar shuffle
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    m = fmaxf(m, __uint_as_float(sw[1]));
    m += eb;
    if (h == 0) out[static_cast<int64_t>(glob_of(cg)) * 32 + r32] = m;
  };
  // Software pipeline, one candidate per step: step c issues candidate c's MFMA chain and, in the
  // same basic block, the independent VALU work of later candidates (the operands of c + 1, and at
  // every other step the w rows of c + 2 and c + 3, so the operands of c + 1 need no w row of the
  // same step), which the scheduler places between the MFMAs; kNN rows are loaded six candidates
  // ahead (they come from HBM / the infinity cache), gathered rows two ahead of their use.  Slots:
  // rows U & 7, w rows U & 3, gathered rows and operands U & 1 (unrolled by 8, so every slot index
  // is a constant).  The operands of c + 1 are not pinned before step c's exit test: the compiler
  // sinks part of their computation into step c + 1, which measured faster (three waves per SIMD
  // overlap one wave's chain with another's VALU better than one wave interleaves both).
  float dj[8];
  int nn[8];
  Gathered G[2];
  Prepared X[2];
  Cand t0 = cand_at(g), t2 = cand_at(g + 2 * stride), t6 = cand_at(g + 6 * stride);
  {
    Cand r = t0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      load_row(r, dj[i], nn[i]);
      advance(r);
    }
    Cand c1 = t0;
    advance(c1);
    gather(t0, nn[0], G[0]);
    gather(c1, nn[1], G[1]);
    weights2(dj[0], dj[1], 0, 1);
    prep(G[0], 0, X[0]);
  }
#define DVCP_DFE_STEP(U)                                            \
  {                                                                 \
    const f32x16 acc = mfma(X[(U)&1]);                              \
    prep(G[((U) + 1) & 1], ((U) + 1) & 3, X[((U) + 1) & 1]);        \
    if (((U)&1) == 0)                                               \
      weights2(dj[((U) + 2) & 7], dj[((U) + 3) & 7], ((U) + 2) & 3, \
               ((U) + 3) & 3);                                      \
    load_row(t6, dj[((U) + 6) & 7], nn[((U) + 6) & 7]);             \
    gather(t2, nn[((U) + 2) & 7], G[(U)&1]);                        \
    finish(t0, acc);                                                \
    advance(t0);                                                    \
    advance(t2);                                                    \
    advance(t6);                                                    \
    if (t0.li >= total) break;                                      \
  }
  for (;;) {
    DVCP_DFE_STEP(0)
    DVCP_DFE_STEP(1)
    DVCP_DFE_STEP(2)
    DVCP_DFE_STEP(3)
    DVCP_DFE_STEP(4)
    DVCP_DFE_STEP(5)
    DVCP_DFE_STEP(6)
    DVCP_DFE_STEP(7)
  }
#undef DVCP_DFE_STEP
}

template <typename T, typename FT>
int launch_dfe_tgt_mfma(PointsView<T> ref, const FT* feat, int M, const float* cand, const float* dist,
                        const int32_t* idx, int B, int Q, const float* params, float* out, bool literal,
                        hipStream_t st) {
  constexpr bool kF32 = std::is_same<FT, float>::value;
  const int64_t total = static_cast<int64_t>(B) * Q;
  if (total >= (int64_t(1) << 31) / 32) {
    set_error("%s: B*Q=%lld too large", kF32 ? "dvcp_dfe_tgt" : "dvcp_dfe_tgt_f16", static_cast<long long>(total));
    return DVCP_EINVAL;
  }
  const int64_t need = (total + kDfeMfmaWaves - 1) / kDfeMfmaWaves;
  if constexpr (kF32) {
    if (literal) {
      dfe_tgt_literal_launch<T>(need, st, ref, feat, M, cand, dist, idx, Q, B, params, out);
      return launch_status("dvcp_dfe_tgt(mfma)");
    }
  }
  // a few resident workgroups per CU amortise the fp64 prologue over many candidates
  const int xcd = B % 8 == 0 && need >= kDfeGrid ? 1 : 0;  // equal pairs per XCD
  const int grid = static_cast<int>(need < kDfeGrid ? need : kDfeGrid);
  if (sizeof(T) == 4 && ref.rows4())
    hipLaunchKernelGGL((dfe_tgt_mfma1_kernel<T, FT, sizeof(T) == 4>), dim3(grid), dim3(kDfe1Waves * kWave), 0, st, ref,
                       feat, M, cand, dist, idx, Q, B, params, out, xcd);
  else
    hipLaunchKernelGGL((dfe_tgt_mfma1_kernel<T, FT>), dim3(grid), dim3(kDfe1Waves * kWave), 0, st, ref, feat, M, cand,
                       dist, idx, Q, B, params, out, xcd);
  return launch_status(kF32 ? "dvcp_dfe_tgt(mfma)" : "dvcp_dfe_tgt_f16");
}

template int launch_dfe_tgt_mfma<float, float>(PointsView<float>, const float*, int, const float*, const float*,
                                               const int32_t*, int, int, const float*, float*, bool, hipStream_t);
template int launch_dfe_tgt_mfma<double, float>(PointsView<double>, const float*, int, const float*, const float*,
                                                const int32_t*, int, int, const float*, float*, bool, hipStream_t);

}  // namespace dvcp

// The fp16-feature table (C5): the collapsed kernel only.
extern "C" int dvcp_dfe_tgt_f16(int dtype, const void* ref_xyz, int64_t rb, int64_t rc, int64_t rn, int M,
                                const uint16_t* ref_feat, const float* cand, const float* dist, const int32_t* idx,
                                int B, int Q, const float* params, float* out, void* stream) {
  DVCP_REQUIRE(ref_xyz && ref_feat && cand && dist && idx && params && out, "dvcp_dfe_tgt_f16: null pointer");
  DVCP_REQUIRE(M > 0 && B >= 0 && B <= 65535 && Q >= 0, "dvcp_dfe_tgt_f16: bad sizes");
  if (B == 0 || Q == 0) return DVCP_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const _Float16* f = reinterpret_cast<const _Float16*>(ref_feat);
  if (dtype == DVCP_F32)
    return dvcp::launch_dfe_tgt_mfma(dvcp::PointsView<float>{static_cast<const float*>(ref_xyz), rb, rc, rn}, f, M,
                                     cand, dist, idx, B, Q, params, out, false, st);
  if (dtype == DVCP_F64)
    return dvcp::launch_dfe_tgt_mfma(dvcp::PointsView<double>{static_cast<const double*>(ref_xyz), rb, rc, rn}, f, M,
                                     cand, dist, idx, B, Q, params, out, false, st);
  dvcp::set_error("dvcp_dfe_tgt_f16: bad dtype %d", dtype);
  return DVCP_EINVAL;
}
