// Grouped expert GEMMs for routed MoE blocks on gfx950 (Qwen3-MoE serving).
//
// moe.hip sorts the T·k (token, expert) pairs into contiguous per-expert segments (perm, offsets).  The two
// kernels here run the expert MLP over all segments in one launch each, with nothing read back to the host:
//
//   stage 0 (swiglu): hs[p, n] = bf16(silu(g) · u),  g = x[perm[p]/k] · w13[e, n]ᵀ,  u = x[perm[p]/k] · w13[e, I + n]ᵀ
//   stage 1 (down):   ys[p, n] = bf16(hs[p] · w2[e, n]ᵀ)
//
// for p in [offsets[e], offsets[e+1]).  The gather of x is folded into the operand addressing (no xs copy) and
// SwiGLU runs on the fp32 accumulators, so a workgroup always holds the gate and the up rows of the same
// output columns.  Both kernels accumulate a pair's K loop in ascending 32-wide MFMA steps into one
// accumulator (v_mfma_f32_16x16x32_bf16, W fragment = A operand, activation rows = B operand), so an output
// row depends only on its own input row and its expert's weights: not on the rows it shares a tile with, its
// place in the segment, or P.  No atomics, no split-K.
//
// Two row classes, picked on the host from (P, E) alone (moe_gemm_class) so that a captured graph is valid
// for every routing:
//
//  * skinny (decode: a handful of rows per expert; the cost is streaming each live expert's weights once).
//    Grid E × ceil(N/128): blockIdx gives (expert, weight-row block) directly and a workgroup whose expert
//    has no rows returns at once.  As in skinny.hip a wave's two 16-row W fragments come straight from HBM
//    with 16-byte loads, eight k-steps in flight; the expert's rows are the B operands of up to four 16-row
//    m-tiles (1, 2 or 4 by the segment's size, a wave-uniform branch on the device).  Longer segments loop
//    over groups of 64 rows and re-read W from L2.
//  * tiled (prefill: tens to hundreds of rows per expert).  64-row × 128-weight-row tiles, BK = 64.  The grid
//    is (min(P, P/64 + E) row tiles) × ceil(N/128); every wave scans ceil(c_e/64) over the E <= 128 experts
//    (two per lane, shuffle prefix sum) to find its (expert, row tile); tiles past the total return at once.
//    W and the gathered activation rows go global → LDS by LDS-DMA (global_load_lds_dwordx4, per-lane global
//    addresses, so the gather costs nothing), double buffered.  The DMA writes lane l of a wave to slot l of
//    a 1-KiB run, so the XOR swizzle that keeps the 16-row fragment reads off the same banks is applied on
//    the global side: slot s of row r holds 16-B chunk s ^ (r & 7).  Ragged last row tiles and ragged N
//    blocks are clamped on load and masked on store, never padded in memory.
//
// FP8 expert weights (W8A16; moe_gemm_*_fp8_k).  W holds e4m3 codes with one fp32 scale per (expert, weight row),
// quantised by quant/fp8.py::quantize_rows_reference; activations stay bf16.  Every finite e4m3 value is exact in
// bf16, so the codes are converted in registers (v_cvt_pk_f32_fp8, then the upper halves) and go through the same
// v_mfma_f32_16x16x32_bf16; the scale multiplies the fp32 accumulator in the epilogue (g and u separately, before
// SwiGLU; their scales sit I rows apart), so a weight is never rounded a second time.  Grids, row classes, the
// ascending K loop into one accumulator and the row-invariance of the bf16 kernels are kept; H % 64 == I % 64 == 0.
//
//  * skinny: a lane's 16-byte load is 16 codes = its A operand of TWO 32-deep k-steps.  Lane group g of row li
//    reads bytes 64s + 16g .. + 15; codes 0..7 feed step 2s, codes 8..15 step 2s + 1, and x is read with the same
//    address function (k = 64s + 16g + 8h + i), which is all a dot product needs.  Eight loads per fragment stay
//    in flight as before, so one batch covers 512 of K instead of 256; conversion runs under the next loads.
//  * tiled: LDS-DMA moves bytes and cannot convert, so a W stage (128 rows × 64 codes = 8 KiB, half the bf16
//    bytes) goes global → registers one stage ahead, is converted ONCE per workgroup (two 16-byte loads, two cvt16
//    and four ds_write_b128 per thread) and is written as the same swizzled bf16 image; fragment reads and the
//    MFMA loop are those of the bf16 kernel.  The gathered x rows keep going by LDS-DMA.
//
// Backward with frozen experts (moe_gemm_nn_k; fine-tuning with adapters elsewhere, base weights frozen).  Under
// autograd the SwiGLU stage also writes gu [P, 2I] = bf16(g), bf16(u) from the same epilogue (template parameter GU;
// hs still comes from the unrounded accumulators, so the forward bits do not change), and the input gradient is two
// launches of one NN kernel, out[p, n] = Σ_k A[p, k] · W[e][k][n] with W row-major in n, i.e. the checkpoint layouts
// w2 [E, H, I] and w13 [E, 2I, H] read as they are:
//
//   dswiglu: dh = dys[p] · w2[e] (K = H, N = I), never stored; with s = 1 / (1 + exp(-g)):
//            dgu[p, n] = bf16(dh·u·s·(1 + g·(1 - s))),  dgu[p, I + n] = bf16(dh·g·s)
//   dx:      dxs[p, n] = bf16(dgu[p] · w13[e]) (K = 2I, N = H); moe_combine then sums a token's k rows.
//
// One tiled class for every P: the forward's 64-row × 128-column tiles, BK = 64, 2 × 2 waves, grid and find_tile scan,
// LDS-DMA double buffering with one barrier per stage, K ascending into one accumulator, no atomics, no split-K, and
// the same row invariance (a dxs row depends on its dys and gu rows and its expert's weights only).  What differs is
// the W stage: 64 k-rows × 128 columns (256 B per k-row, 16 KiB), so a wave DMA instruction fills 4 k-rows.  The MFMA
// keeps the weight fragment as its A operand, which wants 8 consecutive k at a fixed n per lane; the image has n
// contiguous, so a fragment is two ds_read_b64_tr_b16: lane (g, kq, kp) of a k-step reads 8 bytes of k-row 8g + kq
// (then + 4) at columns 4·kp .. + 3 of the fragment's 32-B column pair, and receives k-rows 8g .. 8g + 3 (+ 4) of
// column li.  Swizzle: pair c of k-row k sits at pair c ^ h(k), h(k) = (k & 3) | ((k >> 1) & 4), applied on the global
// source address (slot ch of a DMA'd k-row ← 16-B chunk ch ^ 2·h(k), which keeps a pair's halves in place).  Why it
// is conflict-free: LDS serves a 64-bit wave read in two halves of 32 lanes; a half is g ∈ {2m, 2m + 1}, kq ∈ 0..3,
// i.e. the 8 k-rows {16m .. 16m + 3, 16m + 8 .. 16m + 11} (+ 4 for the second read), 32 contiguous bytes each.  Every
// k-row starts on bank 0 (256-B rows, 64 banks × 4 B), so unswizzled all 8 would hit the same 8 banks; h takes the 8
// values kq | 4·(g & 1) on them, so the 8 rows land in 8 distinct 32-B bank slots and cover the 64 banks once.  The
// DMA's own writes are 1 KiB contiguous whatever the source.  K is never ragged (H % 64 == 2I % 64 == 0); ragged N
// (I or H not a multiple of 128) is clamped per 16-B chunk on load and masked on store.
//
// Backward over FP8 codes (moe_gemm_nn_fp8_k; frozen e4m3 experts under adapters).  The forward FP8 kernels take the
// same GU parameter (gu = the scaled fp32 accumulators rounded once; hs still from the unrounded values).  The NN
// kernel above is kept whole (tiles, grid, find_tile, A rows by LDS-DMA, transposed fragment reads with woff, the
// image and its swizzle, ascending K, row invariance) except for the W stage, which is the codes c2 [E, H, I] and
// c13 [E, 2I, H] as they are: 64 k-rows × 128 codes = 8 KiB, global → registers one stage ahead as in
// moe_gemm_tiled_fp8_k, converted once per workgroup.  Thread tid loads 16 codes of k-row tid / 8 (and + 32) at source
// column min(n0 + 16·m, N − 16), m = tid % 8 (N % 64 == 0: a pair is wholly in or out of the matrix).  16 codes are one
// 32-B column pair of the image, so they become two bf16x8 and two ds_write_b128 at pair m ^ nn_swz(k) of the k-row;
// nn_swz(k + 32) == nn_swz(k), so the second load lands 32 rows further at the same offset.  The writes and the banks:
// a wave holds k-rows 8w .. 8w + 7 (8 lanes each), 256 B per k-row, i.e. one contiguous 2-KiB run of the image; m ↦
// m ^ nn_swz(k) permutes the 8 pairs of a k-row, so the wave's two ds_write_b128 (lower and upper 16 B of every pair)
// together write each of the run's 128 16-B slots exactly once.  The reads are those of the bf16 kernel and the bank
// argument above holds for them unchanged, since the image is the same.
// Where the scales go: both run along the reduction index of their GEMM and cannot meet the accumulator.
//   dswiglu (W = c2, K = H): the conversion multiplies by s2[e, k-row] in fp32 before the bf16 rounding, one scalar per
//            load fetched with the codes: the image holds wq2 = bf16(fp32(val(c2))·s2), the one place where a weight is
//            rounded a second time.  The epilogue multiplies dg by s13[e, n] and du by s13[e, I + n] in fp32 before
//            their single rounding (two more 16-B loads per lane and fragment), which folds the second GEMM's scale.
//   dx      (W = c13, K = 2I): plain cvt16 over the exact code values, no scale anywhere.
#include "common.h"

using namespace lipa;

namespace {

constexpr int MG_KS = 8;      // skinny: k-steps (of 32) per load batch
constexpr int MG_BM = 64;     // tiled: rows per tile
constexpr int MG_BN = 128;    // weight rows per workgroup (both classes); swiglu: 64 gate + 64 up
constexpr int MG_BK = 64;     // tiled: K per LDS stage

__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.f + __expf(-g)) * u; }

__device__ __forceinline__ void store4(bf16* p, float a, float b, float c, float d) {
  bf16x4 o;
  o[0] = (bf16)a; o[1] = (bf16)b; o[2] = (bf16)c; o[3] = (bf16)d;
  *reinterpret_cast<bf16x4*>(p) = o;
}

// Epilogue shared by both classes.  acc[j] holds C[n = nrow[j] + 4g + i][row]; SWIGLU: j = 0 gate, j = 1 up of
// the same logical columns → one 8-byte store; DOWN: one 8-byte store per fragment.  GU (SWIGLU under autograd): g and
// u themselves, the fp32 accumulators rounded once, also go to gu [P, 2·ldo] (g in columns 0..I-1, u in I..2I-1);
// hs is still computed from the unrounded accumulators.
template <bool SWIGLU, bool GU = false>
__device__ __forceinline__ void store_pair(bf16* out, int ldo, int p, int col0, int col1, const f32x4& a0,
                                           const f32x4& a1, bf16* gu = nullptr) {
  bf16* o = out + (size_t)p * ldo;
  if (GU) {
    bf16* q = gu + (size_t)p * 2 * ldo + col0;
    store4(q, a0[0], a0[1], a0[2], a0[3]);
    store4(q + ldo, a1[0], a1[1], a1[2], a1[3]);
  }
  if (SWIGLU) {
    store4(o + col0, silu_mul(a0[0], a1[0]), silu_mul(a0[1], a1[1]), silu_mul(a0[2], a1[2]), silu_mul(a0[3], a1[3]));
  } else {
    store4(o + col0, a0[0], a0[1], a0[2], a0[3]);
    store4(o + col1, a1[0], a1[1], a1[2], a1[3]);
  }
}

// ------------------------------------------------------------------ skinny
// One group of up to 16·MT rows [r0, r1) of the segment against this wave's two W fragments.
template <bool SWIGLU, bool GU, int MT>
__device__ __forceinline__ void skinny_rows(const bf16* __restrict__ A, const int* __restrict__ perm, int kdiv,
                                            const bf16* wr0, const bf16* wr1, bf16* __restrict__ out,
                                            bf16* __restrict__ gu, int ldo, int K, int r0, int r1, int col0,
                                            int col1) {
  const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
  const bf16* xr[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int p = min(r0 + 16 * mt + li, r1 - 1);
    xr[mt] = A + (size_t)(perm ? perm[p] / kdiv : p) * K + 8 * g;
  }
  f32x4 acc[2][MT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < K; kb += 32 * MG_KS) {
    const int ns = min(MG_KS, (K - kb) / 32);
    bf16x8 a0[MG_KS], a1[MG_KS];
#pragma unroll
    for (int s = 0; s < MG_KS; ++s)
      if (s < ns) {
        a0[s] = *reinterpret_cast<const bf16x8*>(wr0 + kb + 32 * s);
        a1[s] = *reinterpret_cast<const bf16x8*>(wr1 + kb + 32 * s);
      }
#pragma unroll
    for (int s = 0; s < MG_KS; ++s)
      if (s < ns) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(xr[mt] + kb + 32 * s);
          acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[s], b, acc[0][mt], 0, 0, 0);
          acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[s], b, acc[1][mt], 0, 0, 0);
        }
      }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int p = r0 + 16 * mt + li;
    if (p < r1) store_pair<SWIGLU, GU>(out, ldo, p, col0 + 4 * g, col1 + 4 * g, acc[0][mt], acc[1][mt], gu);
  }
}

// A [rows, K] (x through perm for SWIGLU, hs for DOWN); W [E, NW, K] with NW = 2N (SWIGLU) or N (DOWN);
// out [P, N]; GU: gu [P, 2N] as well.  grid = E · ceil(N / (SWIGLU ? 64 : 128)).
template <bool SWIGLU, bool GU = false>
__global__ __launch_bounds__(256) void moe_gemm_skinny_k(const bf16* __restrict__ A, const int* __restrict__ perm,
                                                         int kdiv, const int* __restrict__ offsets,
                                                         const bf16* __restrict__ W, bf16* __restrict__ out,
                                                         bf16* __restrict__ gu, int N, int K, int nblk) {
  const int e = blockIdx.x / nblk, bn = blockIdx.x % nblk;
  const int s0 = offsets[e], s1 = offsets[e + 1];
  if (s1 <= s0) return;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
  // SWIGLU: 16 logical columns per wave (fragment 0 = gate rows, 1 = up rows); DOWN: 32 columns per wave
  const int col0 = SWIGLU ? bn * 64 + 16 * w : bn * 128 + 32 * w;
  const int col1 = SWIGLU ? col0 : col0 + 16;
  if (col0 >= N) return;                    // N % 32 == 0 (SWIGLU: % 16): a wave is wholly in or out
  const bf16* We = W + (size_t)e * (SWIGLU ? 2 : 1) * N * K;
  const bf16* wr0 = We + (size_t)(col0 + li) * K + 8 * g;
  const bf16* wr1 = We + (size_t)((SWIGLU ? N + col0 : col1) + li) * K + 8 * g;
  for (int r0 = s0; r0 < s1; r0 += 64) {
    const int r1 = min(s1, r0 + 64), n = r1 - r0;
    if (n <= 16) skinny_rows<SWIGLU, GU, 1>(A, perm, kdiv, wr0, wr1, out, gu, N, K, r0, r1, col0, col1);
    else if (n <= 32) skinny_rows<SWIGLU, GU, 2>(A, perm, kdiv, wr0, wr1, out, gu, N, K, r0, r1, col0, col1);
    else skinny_rows<SWIGLU, GU, 4>(A, perm, kdiv, wr0, wr1, out, gu, N, K, r0, r1, col0, col1);
  }
}

// ------------------------------------------------------------------ tiled
typedef __attribute__((address_space(3))) void* lds_ptr;
typedef const __attribute__((address_space(1))) void* glb_ptr;

// 16 bytes per lane, global → LDS: lane l lands at lds + 16·l (lds is wave-uniform)
__device__ __forceinline__ void dma16(const bf16* gsrc, bf16* lds) {
  __builtin_amdgcn_global_load_lds((glb_ptr)gsrc, (lds_ptr)lds, 16, 0, 0);
}

// Tile t of the launch → (expert, first row, segment end); false when t is past the last tile.  Each lane
// holds experts 2l and 2l+1; an inclusive shuffle scan of their tile counts orders the tiles by expert.
__device__ __forceinline__ bool find_tile(const int* __restrict__ offsets, int E, int t, int& e, int& r0, int& s1) {
  const int lane = threadIdx.x & 63;
  const int ea = 2 * lane, eb = ea + 1;
  const int o0 = offsets[min(ea, E)], o1 = offsets[min(eb, E)], o2 = offsets[min(eb + 1, E)];
  const int ca = (o1 - o0 + MG_BM - 1) / MG_BM, cb = (o2 - o1 + MG_BM - 1) / MG_BM;
  int incl = ca + cb;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  const int excl = incl - ca - cb;
  const bool hit = t >= excl && t < incl;
  const uint64_t bal = __ballot(hit);
  if (bal == 0) return false;
  const int src = __ffsll((unsigned long long)bal) - 1;
  const bool second = t >= excl + ca;
  const int me = second ? eb : ea;
  const int mr = (second ? o1 : o0) + (t - excl - (second ? ca : 0)) * MG_BM;
  const int ms = second ? o2 : o1;
  e = __shfl(me, src, 64);
  r0 = __shfl(mr, src, 64);
  s1 = __shfl(ms, src, 64);
  return true;
}

template <bool SWIGLU, bool GU = false>
__global__ __launch_bounds__(256) void moe_gemm_tiled_k(const bf16* __restrict__ A, const int* __restrict__ perm,
                                                        int kdiv, const int* __restrict__ offsets,
                                                        const bf16* __restrict__ W, bf16* __restrict__ out,
                                                        bf16* __restrict__ gu, int E, int N, int K, int nblk) {
  __shared__ __attribute__((aligned(16))) bf16 sx[2][MG_BM * MG_BK];
  __shared__ __attribute__((aligned(16))) bf16 sw[2][MG_BN * MG_BK];
  int e, r0, s1;
  if (!find_tile(offsets, E, blockIdx.x / nblk, e, r0, s1)) return;
  const int bn = blockIdx.x % nblk;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const int wm = w >> 1, wn = w & 1;          // 2 × 2 waves: 32 rows × 64 weight rows each
  const int cols = SWIGLU ? 64 : 128;         // logical output columns per workgroup
  const bf16* We = W + (size_t)e * (SWIGLU ? 2 : 1) * N * K;

  // DMA sources.  A wave instruction fills 8 rows × 8 slots; row r, slot s ← chunk s ^ (r & 7) of that row.
  const int sl = lane & 7;
  const bf16* xsrc[2];
  int xchk[2], wchk[4];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = (q * 4 + w) * 8 + (lane >> 3);
    const int p = min(r0 + r, s1 - 1);
    xsrc[q] = A + (size_t)(perm ? perm[p] / kdiv : p) * K;
    xchk[q] = 8 * (sl ^ (r & 7));
  }
  const bf16* wsrc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = (q * 4 + w) * 8 + (lane >> 3);          // tile row 0..127
    int n;                                                // row of this expert's weight matrix
    if (SWIGLU) n = (r >= 64 ? N : 0) + min(bn * 64 + (r & 63), N - 1);
    else n = min(bn * 128 + r, N - 1);
    wsrc[q] = We + (size_t)n * K;
    wchk[q] = 8 * (sl ^ (r & 7));
  }
  // K % 64 == 32 (I = 96): the last stage is half wide; its upper chunks re-read the lower ones (in bounds, unused)
  auto koff = [&](int k0, int chk) { return k0 + chk < K ? k0 + chk : k0 + chk - 32; };
  auto issue = [&](int buf, int k0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) dma16(xsrc[q] + koff(k0, xchk[q]), &sx[buf][(q * 4 + w) * 8 * MG_BK]);
#pragma unroll
    for (int q = 0; q < 4; ++q) dma16(wsrc[q] + koff(k0, wchk[q]), &sw[buf][(q * 4 + w) * 8 * MG_BK]);
  };

  // fragment j of this wave → tile row of W.  SWIGLU: j = 2c + {0 gate, 1 up} for column group c = 0, 1
  int frow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) frow[j] = SWIGLU ? (j & 1) * 64 + wn * 32 + (j >> 1) * 16 : wn * 64 + 16 * j;

  f32x4 acc[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) acc[j][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (K + MG_BK - 1) / MG_BK;
  issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this lane's part of stage kt has landed
    __syncthreads();                                        // stage kt visible; every wave is done reading stage kt-1
    if (kt + 1 < nk) issue(buf ^ 1, (kt + 1) * MG_BK);      // flies under this stage's MFMAs
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (kt * MG_BK + 32 * ks >= K) break;
      const int c = ks * 4 + g;
      bf16x8 b[2], a[4];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int r = wm * 32 + mi * 16 + li;
        b[mi] = *reinterpret_cast<const bf16x8*>(&sx[buf][r * MG_BK + 8 * (c ^ (r & 7))]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = frow[j] + li;
        a[j] = *reinterpret_cast<const bf16x8*>(&sw[buf][r * MG_BK + 8 * (c ^ (r & 7))]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
          acc[j][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[mi], acc[j][mi], 0, 0, 0);
    }
  }

#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int p = r0 + wm * 32 + mi * 16 + li;
    if (p >= s1) continue;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      // SWIGLU: fragments (2c, 2c+1) = gate / up of columns wn·32 + 16c; DOWN: columns wn·64 + 32c (+16)
      const int col0 = bn * cols + (SWIGLU ? wn * 32 + 16 * c : wn * 64 + 32 * c) + 4 * g;
      if (col0 >= N) continue;
      store_pair<SWIGLU, GU>(out, N, p, col0, col0 + 16, acc[2 * c][mi], acc[2 * c + 1][mi], gu);
    }
  }
}

// ================================================================== backward with frozen experts: NN grouped GEMMs
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// W image swizzle: the 32-B column pair c of k-row k sits at pair c ^ nn_swz(k) of the row's 8 pairs
__device__ __forceinline__ int nn_swz(int k) { return (k & 3) | ((k >> 1) & 4); }

// out[p, n] = Σ_k A[p, k] · W[e][k][n] for p in expert e's segment: A [P, K], W [E, K, N] with n contiguous.
//   DSWIGLU (A = dys, W = w2, K = H, N = I): acc = dh, never stored; with g, u = gu[p, n], gu[p, N + n] and
//     s = 1 / (1 + exp(-g)):  out[p, n] = bf16(dh·u·s·(1 + g·(1 - s))),  out[p, N + n] = bf16(dh·g·s);  out [P, 2N].
//   else (A = dgu, W = w13, K = 2I, N = H): out[p, n] = bf16(acc);  out [P, N].
// grid = (row tiles of find_tile) × ceil(N / 128); K % 64 == 0, N % 32 == 0.
template <bool DSWIGLU>
__global__ __launch_bounds__(256) void moe_gemm_nn_k(const bf16* __restrict__ A, const int* __restrict__ offsets,
                                                     const bf16* __restrict__ W, const bf16* __restrict__ gu,
                                                     bf16* __restrict__ out, int E, int N, int K, int nblk) {
  __shared__ __attribute__((aligned(16))) bf16 sx[2][MG_BM * MG_BK];
  __shared__ __attribute__((aligned(16))) bf16 sw[2][MG_BK * MG_BN];
  int e, r0, s1;
  if (!find_tile(offsets, E, blockIdx.x / nblk, e, r0, s1)) return;
  const int n0 = (blockIdx.x % nblk) * MG_BN;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const int wm = w >> 1, wn = w & 1;          // 2 × 2 waves: 32 rows × 64 output columns each
  const bf16* We = W + (size_t)e * K * N;

  // DMA sources.  A: as the forward (8 rows × 8 slots per wave instruction, slot s of row r ← chunk s ^ (r & 7)).
  // W: a wave instruction fills 4 k-rows × 16 slots; slot ch of k-row kr ← 16-B chunk ch ^ 2·nn_swz(kr) of the
  // workgroup's 128 columns, clamped into the row when N is ragged (those columns are masked on store).
  const bf16* xsrc[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = (q * 4 + w) * 8 + (lane >> 3);
    const int p = min(r0 + r, s1 - 1);
    xsrc[q] = A + (size_t)p * K + 8 * ((lane & 7) ^ (r & 7));
  }
  const bf16* wsrc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int kr = (q * 4 + w) * 4 + (lane >> 4);
    const int cc = (lane & 15) ^ (2 * nn_swz(kr));
    wsrc[q] = We + (size_t)kr * N + min(n0 + 8 * cc, N - 8);
  }
  auto issue = [&](int buf, int k0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) dma16(xsrc[q] + k0, &sx[buf][(q * 4 + w) * 8 * MG_BK]);
#pragma unroll
    for (int q = 0; q < 4; ++q) dma16(wsrc[q] + (size_t)k0 * N, &sw[buf][(q * 4 + w) * 4 * MG_BN]);
  };

  // transposed fragment reads: lane (g, kq, kp) reads 8 bytes of k-row 8g + kq (and + 4), columns 4·kp .. + 3 of the
  // fragment's pair; nn_swz of both rows, and of the rows 32 further on, is kq | 4·(g & 1)
  const int kq = (lane >> 2) & 3, kp = lane & 3;
  int woff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) woff[j] = (8 * g + kq) * MG_BN + 16 * ((wn * 4 + j) ^ (kq | ((g & 1) << 2))) + 4 * kp;

  f32x4 acc[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) acc[j][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / MG_BK;
  issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this lane's part of stage kt has landed
    __syncthreads();                                        // stage kt visible; every wave is done reading stage kt-1
    if (kt + 1 < nk) issue(buf ^ 1, (kt + 1) * MG_BK);      // flies under this stage's MFMAs
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = ks * 4 + g;
      bf16x8 b[2], a[4];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int r = wm * 32 + mi * 16 + li;
        b[mi] = *reinterpret_cast<const bf16x8*>(&sx[buf][r * MG_BK + 8 * (c ^ (r & 7))]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16* pw = &sw[buf][ks * 32 * MG_BN + woff[j]];
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)pw);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(pw + 4 * MG_BN));
        a[j] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
          acc[j][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[mi], acc[j][mi], 0, 0, 0);
    }
  }

  // acc[j][mi][i] = C[p = r0 + 32·wm + 16·mi + li][n = n0 + 64·wn + 16·j + 4·g + i]
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int p = r0 + wm * 32 + mi * 16 + li;
    if (p >= s1) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = n0 + wn * 64 + 16 * j + 4 * g;
      if (col >= N) continue;                               // N % 4 == 0: a lane's four columns are in or out together
      const f32x4& dh = acc[j][mi];
      if (DSWIGLU) {
        const size_t at = (size_t)p * 2 * N + col;
        const bf16x4 gv = *reinterpret_cast<const bf16x4*>(gu + at), uv = *reinterpret_cast<const bf16x4*>(gu + at + N);
        float dg[4], du[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float gg = (float)gv[i], uu = (float)uv[i], s = 1.f / (1.f + __expf(-gg));
          dg[i] = dh[i] * uu * s * (1.f + gg * (1.f - s));
          du[i] = dh[i] * gg * s;
        }
        store4(out + at, dg[0], dg[1], dg[2], dg[3]);
        store4(out + at + N, du[0], du[1], du[2], du[3]);
      } else {
        store4(out + (size_t)p * N + col, dh[0], dh[1], dh[2], dh[3]);
      }
    }
  }
}

// ================================================================== FP8 (e4m3) expert weights, W8A16
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int MG8_LS = 8;     // skinny: 16-byte code loads per fragment and batch (16 k-steps, 512 of K)

// 16 e4m3 codes → 2 × 8 bf16, exact (every finite e4m3 value has 3 mantissa bits)
__device__ __forceinline__ void cvt16(const u32x4& c, bf16x8& a, bf16x8& b) {
  float f[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], true);
    f[4 * i] = lo[0]; f[4 * i + 1] = lo[1]; f[4 * i + 2] = hi[0]; f[4 * i + 3] = hi[1];
  }
  a = bf16x8{(bf16)f[0], (bf16)f[1], (bf16)f[2], (bf16)f[3], (bf16)f[4], (bf16)f[5], (bf16)f[6], (bf16)f[7]};
  b = bf16x8{(bf16)f[8], (bf16)f[9], (bf16)f[10], (bf16)f[11], (bf16)f[12], (bf16)f[13], (bf16)f[14], (bf16)f[15]};
}

// the row scales of an accumulator fragment meet the fp32 sum: acc[i] ↔ weight row n0 + i
__device__ __forceinline__ f32x4 scaled(const f32x4& a, const f32x4& s) {
  return f32x4{a[0] * s[0], a[1] * s[1], a[2] * s[2], a[3] * s[3]};
}

// ------------------------------------------------------------------ skinny, codes
// As skinny_rows, with wr0 / wr1 pointing at code bytes.  Lane (li, g) loads bytes 64s + 16g .. + 15 of weight row
// li: codes 0..7 are its A operand of k-step 2s, codes 8..15 of k-step 2s + 1, and the x rows are read at the
// same k (64s + 16g + 8h + i), so both operands of an MFMA step hold the same 32 k-values in the same slots.
template <bool SWIGLU, bool GU, int MT>
__device__ __forceinline__ void skinny8_rows(const bf16* __restrict__ A, const int* __restrict__ perm, int kdiv,
                                             const uint8_t* wr0, const uint8_t* wr1, const f32x4& sc0,
                                             const f32x4& sc1, bf16* __restrict__ out, bf16* __restrict__ gu, int ldo,
                                             int K, int r0, int r1, int col0, int col1) {
  const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
  const bf16* xr[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int p = min(r0 + 16 * mt + li, r1 - 1);
    xr[mt] = A + (size_t)(perm ? perm[p] / kdiv : p) * K + 16 * g;
  }
  f32x4 acc[2][MT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < K; kb += 64 * MG8_LS) {
    const int ns = min(MG8_LS, (K - kb) / 64);
    u32x4 c0[MG8_LS], c1[MG8_LS];
#pragma unroll
    for (int s = 0; s < MG8_LS; ++s)
      if (s < ns) {
        c0[s] = *reinterpret_cast<const u32x4*>(wr0 + kb + 64 * s);
        c1[s] = *reinterpret_cast<const u32x4*>(wr1 + kb + 64 * s);
      }
#pragma unroll
    for (int s = 0; s < MG8_LS; ++s)
      if (s < ns) {
        bf16x8 a0[2], a1[2];
        cvt16(c0[s], a0[0], a0[1]);
        cvt16(c1[s], a1[0], a1[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(xr[mt] + kb + 64 * s + 8 * h);
            acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[h], b, acc[0][mt], 0, 0, 0);
            acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[h], b, acc[1][mt], 0, 0, 0);
          }
      }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int p = r0 + 16 * mt + li;
    if (p < r1)
      store_pair<SWIGLU, GU>(out, ldo, p, col0 + 4 * g, col1 + 4 * g, scaled(acc[0][mt], sc0), scaled(acc[1][mt], sc1),
                             gu);
  }
}

// W [E, NW, K] e4m3 codes, scale fp32 [E, NW]; everything else as moe_gemm_skinny_k (GU: the scaled g and u, rounded
// once, go to gu [P, 2N]).  K % 64 == 0, N % 64 == 0.
template <bool SWIGLU, bool GU = false>
__global__ __launch_bounds__(256) void moe_gemm_skinny_fp8_k(const bf16* __restrict__ A, const int* __restrict__ perm,
                                                             int kdiv, const int* __restrict__ offsets,
                                                             const uint8_t* __restrict__ W,
                                                             const float* __restrict__ scale, bf16* __restrict__ out,
                                                             bf16* __restrict__ gu, int N, int K, int nblk) {
  const int e = blockIdx.x / nblk, bn = blockIdx.x % nblk;
  const int s0 = offsets[e], s1 = offsets[e + 1];
  if (s1 <= s0) return;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
  const int col0 = SWIGLU ? bn * 64 + 16 * w : bn * 128 + 32 * w;
  const int col1 = SWIGLU ? col0 : col0 + 16;
  if (col0 >= N) return;                    // N % 64 == 0: a wave is wholly in or out
  const int NW = (SWIGLU ? 2 : 1) * N, n0 = col0, n1 = SWIGLU ? N + col0 : col1;
  const uint8_t* We = W + (size_t)e * NW * K;
  const float* se = scale + (size_t)e * NW;
  const uint8_t* wr0 = We + (size_t)(n0 + li) * K + 16 * g;
  const uint8_t* wr1 = We + (size_t)(n1 + li) * K + 16 * g;
  const f32x4 sc0 = *reinterpret_cast<const f32x4*>(se + n0 + 4 * g);
  const f32x4 sc1 = *reinterpret_cast<const f32x4*>(se + n1 + 4 * g);
  for (int r0 = s0; r0 < s1; r0 += 64) {
    const int r1 = min(s1, r0 + 64), n = r1 - r0;
    if (n <= 16) skinny8_rows<SWIGLU, GU, 1>(A, perm, kdiv, wr0, wr1, sc0, sc1, out, gu, N, K, r0, r1, col0, col1);
    else if (n <= 32) skinny8_rows<SWIGLU, GU, 2>(A, perm, kdiv, wr0, wr1, sc0, sc1, out, gu, N, K, r0, r1, col0, col1);
    else skinny8_rows<SWIGLU, GU, 4>(A, perm, kdiv, wr0, wr1, sc0, sc1, out, gu, N, K, r0, r1, col0, col1);
  }
}

// ------------------------------------------------------------------ tiled, codes
// As moe_gemm_tiled_k, except for how a W stage reaches LDS: the 128 × 64 code bytes of stage kt + 1 are loaded
// into registers (two 16-byte loads per thread: row tid/4 (+64), quarter tid%4) while stage kt's MFMAs run, are
// converted once, and are written as the two bf16 chunks 2q, 2q + 1 of the swizzled image the DMA would have
// written.  The gathered x rows keep going by LDS-DMA.  One barrier per stage, as before.
template <bool SWIGLU, bool GU = false>
__global__ __launch_bounds__(256) void moe_gemm_tiled_fp8_k(const bf16* __restrict__ A, const int* __restrict__ perm,
                                                            int kdiv, const int* __restrict__ offsets,
                                                            const uint8_t* __restrict__ W,
                                                            const float* __restrict__ scale, bf16* __restrict__ out,
                                                            bf16* __restrict__ gu, int E, int N, int K, int nblk) {
  __shared__ __attribute__((aligned(16))) bf16 sx[2][MG_BM * MG_BK];
  __shared__ __attribute__((aligned(16))) bf16 sw[2][MG_BN * MG_BK];
  int e, r0, s1;
  if (!find_tile(offsets, E, blockIdx.x / nblk, e, r0, s1)) return;
  const int bn = blockIdx.x % nblk;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const int wm = w >> 1, wn = w & 1;
  const int cols = SWIGLU ? 64 : 128;
  const int NW = (SWIGLU ? 2 : 1) * N;
  const uint8_t* We = W + (size_t)e * NW * K;
  const float* se = scale + (size_t)e * NW;

  const int sl = lane & 7;
  const bf16* xsrc[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = (q * 4 + w) * 8 + (lane >> 3);
    const int p = min(r0 + r, s1 - 1);
    xsrc[q] = A + (size_t)(perm ? perm[p] / kdiv : p) * K + 8 * (sl ^ (r & 7));
  }
  const uint8_t* wsrc[2];
  int wdst[2][2];                                           // element offsets of this thread's two chunks in a stage
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = q * 64 + (tid >> 2), c = 2 * (tid & 3);   // tile row 0..127, first of two 8-wide chunks
    int n;
    if (SWIGLU) n = (r >= 64 ? N : 0) + min(bn * 64 + (r & 63), N - 1);
    else n = min(bn * 128 + r, N - 1);
    wsrc[q] = We + (size_t)n * K + 8 * c;
    wdst[q][0] = r * MG_BK + 8 * (c ^ (r & 7));
    wdst[q][1] = r * MG_BK + 8 * ((c + 1) ^ (r & 7));
  }
  u32x4 wreg[2];
  auto issue_x = [&](int buf, int k0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) dma16(xsrc[q] + k0, &sx[buf][(q * 4 + w) * 8 * MG_BK]);
  };
  auto load_w = [&](int k0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) wreg[q] = *reinterpret_cast<const u32x4*>(wsrc[q] + k0);
  };
  auto put_w = [&](int buf) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      bf16x8 lo, hi;
      cvt16(wreg[q], lo, hi);
      *reinterpret_cast<bf16x8*>(&sw[buf][wdst[q][0]]) = lo;
      *reinterpret_cast<bf16x8*>(&sw[buf][wdst[q][1]]) = hi;
    }
  };

  int frow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) frow[j] = SWIGLU ? (j & 1) * 64 + wn * 32 + (j >> 1) * 16 : wn * 64 + 16 * j;

  f32x4 acc[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) acc[j][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / MG_BK;
  issue_x(0, 0);
  load_w(0);
  put_w(0);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this lane's part of x stage kt has landed
    __syncthreads();                                        // stage kt visible; every wave is done reading stage kt-1
    if (kt + 1 < nk) {
      issue_x(buf ^ 1, (kt + 1) * MG_BK);
      load_w((kt + 1) * MG_BK);                             // both fly under this stage's MFMAs
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = ks * 4 + g;
      bf16x8 b[2], a[4];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int r = wm * 32 + mi * 16 + li;
        b[mi] = *reinterpret_cast<const bf16x8*>(&sx[buf][r * MG_BK + 8 * (c ^ (r & 7))]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = frow[j] + li;
        a[j] = *reinterpret_cast<const bf16x8*>(&sw[buf][r * MG_BK + 8 * (c ^ (r & 7))]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
          acc[j][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[mi], acc[j][mi], 0, 0, 0);
    }
    if (kt + 1 < nk) put_w(buf ^ 1);                        // nobody reads that buffer before the next barrier
  }

#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int col0 = bn * cols + (SWIGLU ? wn * 32 + 16 * c : wn * 64 + 32 * c) + 4 * g;
    if (col0 >= N) continue;
    const f32x4 sc0 = *reinterpret_cast<const f32x4*>(se + col0);
    const f32x4 sc1 = *reinterpret_cast<const f32x4*>(se + (SWIGLU ? N + col0 : col0 + 16));
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int p = r0 + wm * 32 + mi * 16 + li;
      if (p >= s1) continue;
      store_pair<SWIGLU, GU>(out, N, p, col0, col0 + 16, scaled(acc[2 * c][mi], sc0), scaled(acc[2 * c + 1][mi], sc1),
                             gu);
    }
  }
}

// ------------------------------------------------------------------ backward over codes: NN grouped GEMM
// 16 e4m3 codes times one fp32 scale → 2 × 8 bf16: bf16(fp32(val)·s), one fp32 multiply and one rounding to nearest even
__device__ __forceinline__ void cvt16_scaled(const u32x4& c, float s, bf16x8& a, bf16x8& b) {
  float f[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], true);
    f[4 * i] = lo[0] * s; f[4 * i + 1] = lo[1] * s; f[4 * i + 2] = hi[0] * s; f[4 * i + 3] = hi[1] * s;
  }
  a = bf16x8{(bf16)f[0], (bf16)f[1], (bf16)f[2], (bf16)f[3], (bf16)f[4], (bf16)f[5], (bf16)f[6], (bf16)f[7]};
  b = bf16x8{(bf16)f[8], (bf16)f[9], (bf16)f[10], (bf16)f[11], (bf16)f[12], (bf16)f[13], (bf16)f[14], (bf16)f[15]};
}

// moe_gemm_nn_k over e4m3 codes W [E, K, N] (n contiguous), read as they are; A, tiles, grid, fragment reads, MFMA loop
// and row invariance as there.  The W stage of kt + 1 (64 k-rows × 128 codes) is loaded into registers while stage kt's
// MFMAs run (two 16-byte loads per thread: k-row tid / 8 (+ 32), column pair tid % 8), converted once and written as
// pair m ^ nn_swz(k) of the swizzled bf16 image the DMA of the bf16 kernel would have written.
//   DSWIGLU (A = dys, W = c2, K = H, N = I): kscale = s2 [E, K] multiplies the code values of its k-row before the bf16
//     rounding (the image is wq2); nscale = s13 [E, 2N] multiplies dg (columns n) and du (columns N + n) in fp32 before
//     their one rounding.  out [P, 2N].
//   else (A = dgu', W = c13, K = 2I, N = H): the exact code values, no scale.  out [P, N].
// K % 64 == 0, N % 64 == 0.
template <bool DSWIGLU>
__global__ __launch_bounds__(256) void moe_gemm_nn_fp8_k(const bf16* __restrict__ A, const int* __restrict__ offsets,
                                                         const uint8_t* __restrict__ W,
                                                         const float* __restrict__ kscale,
                                                         const float* __restrict__ nscale, const bf16* __restrict__ gu,
                                                         bf16* __restrict__ out, int E, int N, int K, int nblk) {
  __shared__ __attribute__((aligned(16))) bf16 sx[2][MG_BM * MG_BK];
  __shared__ __attribute__((aligned(16))) bf16 sw[2][MG_BK * MG_BN];
  int e, r0, s1;
  if (!find_tile(offsets, E, blockIdx.x / nblk, e, r0, s1)) return;
  const int n0 = (blockIdx.x % nblk) * MG_BN;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const int wm = w >> 1, wn = w & 1;          // 2 × 2 waves: 32 rows × 64 output columns each

  const bf16* xsrc[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = (q * 4 + w) * 8 + (lane >> 3);
    const int p = min(r0 + r, s1 - 1);
    xsrc[q] = A + (size_t)p * K + 8 * ((lane & 7) ^ (r & 7));
  }
  // W: k-rows kr and kr + 32 of a stage, 16 codes of column pair m, clamped into the row when N is ragged (those
  // columns are masked on store); both land at pair m ^ nn_swz(kr) of their k-row
  const int kr = tid >> 3, m = tid & 7;
  const uint8_t* wsrc = W + ((size_t)e * K + kr) * N + min(n0 + 16 * m, N - 16);
  const float* ksrc = DSWIGLU ? kscale + (size_t)e * K + kr : nullptr;
  const int wdst = kr * MG_BN + 16 * (m ^ nn_swz(kr));
  u32x4 wreg[2];
  float ksc[2];
  auto issue_x = [&](int buf, int k0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) dma16(xsrc[q] + k0, &sx[buf][(q * 4 + w) * 8 * MG_BK]);
  };
  auto load_w = [&](int k0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      wreg[q] = *reinterpret_cast<const u32x4*>(wsrc + (size_t)(k0 + 32 * q) * N);
      if (DSWIGLU) ksc[q] = ksrc[k0 + 32 * q];
    }
  };
  auto put_w = [&](int buf) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      bf16x8 lo, hi;
      if (DSWIGLU) cvt16_scaled(wreg[q], ksc[q], lo, hi);
      else cvt16(wreg[q], lo, hi);
      bf16* dst = &sw[buf][q * 32 * MG_BN + wdst];
      *reinterpret_cast<bf16x8*>(dst) = lo;
      *reinterpret_cast<bf16x8*>(dst + 8) = hi;
    }
  };

  const int kq = (lane >> 2) & 3, kp = lane & 3;
  int woff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) woff[j] = (8 * g + kq) * MG_BN + 16 * ((wn * 4 + j) ^ (kq | ((g & 1) << 2))) + 4 * kp;

  f32x4 acc[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) acc[j][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / MG_BK;
  issue_x(0, 0);
  load_w(0);
  put_w(0);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this lane's part of A stage kt has landed
    __syncthreads();                                        // stage kt visible; every wave is done reading stage kt-1
    if (kt + 1 < nk) {
      issue_x(buf ^ 1, (kt + 1) * MG_BK);
      load_w((kt + 1) * MG_BK);                             // both fly under this stage's MFMAs
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = ks * 4 + g;
      bf16x8 b[2], a[4];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int r = wm * 32 + mi * 16 + li;
        b[mi] = *reinterpret_cast<const bf16x8*>(&sx[buf][r * MG_BK + 8 * (c ^ (r & 7))]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16* pw = &sw[buf][ks * 32 * MG_BN + woff[j]];
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)pw);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(pw + 4 * MG_BN));
        a[j] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
          acc[j][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[mi], acc[j][mi], 0, 0, 0);
    }
    if (kt + 1 < nk) put_w(buf ^ 1);                        // nobody reads that buffer before the next barrier
  }

  // acc[j][mi][i] = C[p = r0 + 32·wm + 16·mi + li][n = n0 + 64·wn + 16·j + 4·g + i]
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = n0 + wn * 64 + 16 * j + 4 * g;
    if (col >= N) continue;                                 // N % 4 == 0: a lane's four columns are in or out together
    f32x4 sg, su;
    if (DSWIGLU) {
      const float* se = nscale + (size_t)e * 2 * N + col;
      sg = *reinterpret_cast<const f32x4*>(se);
      su = *reinterpret_cast<const f32x4*>(se + N);
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int p = r0 + wm * 32 + mi * 16 + li;
      if (p >= s1) continue;
      const f32x4& dh = acc[j][mi];
      if (DSWIGLU) {
        const size_t at = (size_t)p * 2 * N + col;
        const bf16x4 gv = *reinterpret_cast<const bf16x4*>(gu + at), uv = *reinterpret_cast<const bf16x4*>(gu + at + N);
        float dg[4], du[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float gg = (float)gv[i], uu = (float)uv[i], s = 1.f / (1.f + __expf(-gg));
          dg[i] = dh[i] * uu * s * (1.f + gg * (1.f - s)) * sg[i];
          du[i] = dh[i] * gg * s * su[i];
        }
        store4(out + at, dg[0], dg[1], dg[2], dg[3]);
        store4(out + at + N, du[0], du[1], du[2], du[3]);
      } else {
        store4(out + (size_t)p * N + col, dh[0], dh[1], dh[2], dh[3]);
      }
    }
  }
}

}  // namespace

// Row class from (P, E) alone: 1 = skinny while an average segment fits one 64-row pass twice over, else 2 = tiled.
int moe_gemm_class(int P, int E) { return (long long)P <= 32LL * E ? 1 : 2; }

// stage 0: A = x [T, K=H], perm [P], W = w13 [E, 2N, K], out = hs [P, N=I]
// stage 1: A = hs [P, K=I], perm = nullptr, W = w2 [E, N=H, K], out = ys [P, N]
// gu (stage 0 only, may be null): [P, 2N] bf16, the rounded g and u that the backward reads
void launch_moe_gemm(int stage, int cls, const void* A, const int* perm, int kdiv, const int* offsets, const void* W,
                     void* out, void* gu, int P, int E, int N, int K, hipStream_t st) {
  const int nblk = stage == 0 ? (N + 63) / 64 : (N + 127) / 128;
  const bf16 *a = (const bf16*)A, *wt = (const bf16*)W;
  bf16 *o = (bf16*)out, *q = (bf16*)gu;
  if (cls == 1) {
    const int grid = E * nblk;
    if (stage == 0 && q) moe_gemm_skinny_k<true, true><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, wt, o, q, N, K, nblk);
    else if (stage == 0) moe_gemm_skinny_k<true><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, wt, o, nullptr, N, K, nblk);
    else moe_gemm_skinny_k<false><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, wt, o, nullptr, N, K, nblk);
  } else {
    const int tiles = P < P / MG_BM + E ? P : P / MG_BM + E;     // >= Σ_e ceil(c_e / BM) for every routing
    const int grid = tiles * nblk;
    if (stage == 0 && q) moe_gemm_tiled_k<true, true><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, wt, o, q, E, N, K, nblk);
    else if (stage == 0) moe_gemm_tiled_k<true><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, wt, o, nullptr, E, N, K, nblk);
    else moe_gemm_tiled_k<false><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, wt, o, nullptr, E, N, K, nblk);
  }
  LIPA_CHECK_LAUNCH();
}

// Backward with frozen experts.  stage 0: A = dys [P, K=H], W = w2 [E, K, N=I], gu [P, 2N] → out = dgu [P, 2N];
// stage 1: A = dgu [P, K=2I], W = w13 [E, K, N=H] → out = dxs [P, N].  One tiled class for every P.
void launch_moe_gemm_bwd(int stage, const void* A, const int* offsets, const void* W, const void* gu, void* out, int P,
                         int E, int N, int K, hipStream_t st) {
  const int nblk = (N + MG_BN - 1) / MG_BN;
  const int tiles = P < P / MG_BM + E ? P : P / MG_BM + E;
  const int grid = tiles * nblk;
  if (stage == 0)
    moe_gemm_nn_k<true><<<grid, 256, 0, st>>>((const bf16*)A, offsets, (const bf16*)W, (const bf16*)gu, (bf16*)out, E,
                                              N, K, nblk);
  else
    moe_gemm_nn_k<false><<<grid, 256, 0, st>>>((const bf16*)A, offsets, (const bf16*)W, nullptr, (bf16*)out, E, N, K,
                                               nblk);
  LIPA_CHECK_LAUNCH();
}

// The same two stages over e4m3 codes W with one fp32 scale per (expert, weight row): scale [E, 2N] / [E, N].
// N % 64 == 0 and K % 64 == 0 (a 16-byte code load is half a 64-deep block of one row).  gu as in launch_moe_gemm.
void launch_moe_gemm_fp8(int stage, int cls, const void* A, const int* perm, int kdiv, const int* offsets,
                         const void* W, const float* scale, void* out, void* gu, int P, int E, int N, int K,
                         hipStream_t st) {
  const int nblk = stage == 0 ? (N + 63) / 64 : (N + 127) / 128;
  const bf16* a = (const bf16*)A;
  const uint8_t* Wc = (const uint8_t*)W;
  bf16 *o = (bf16*)out, *q = (bf16*)gu;
  if (cls == 1) {
    const int grid = E * nblk;
    if (stage == 0 && q)
      moe_gemm_skinny_fp8_k<true, true><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, Wc, scale, o, q, N, K, nblk);
    else if (stage == 0)
      moe_gemm_skinny_fp8_k<true><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, Wc, scale, o, nullptr, N, K, nblk);
    else
      moe_gemm_skinny_fp8_k<false><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, Wc, scale, o, nullptr, N, K, nblk);
  } else {
    const int tiles = P < P / MG_BM + E ? P : P / MG_BM + E;
    const int grid = tiles * nblk;
    if (stage == 0 && q)
      moe_gemm_tiled_fp8_k<true, true><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, Wc, scale, o, q, E, N, K, nblk);
    else if (stage == 0)
      moe_gemm_tiled_fp8_k<true><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, Wc, scale, o, nullptr, E, N, K, nblk);
    else
      moe_gemm_tiled_fp8_k<false><<<grid, 256, 0, st>>>(a, perm, kdiv, offsets, Wc, scale, o, nullptr, E, N, K, nblk);
  }
  LIPA_CHECK_LAUNCH();
}

// Backward over the codes, frozen experts.  stage 0: A = dys [P, K=H], W = c2 [E, K, N=I], kscale = s2 [E, K],
// nscale = s13 [E, 2N], gu [P, 2N] → out = dgu' [P, 2N] (s13 folded in); stage 1: A = dgu' [P, K=2I],
// W = c13 [E, K, N=H], no scales → out = dxs [P, N].  One tiled class for every P; N % 64 == 0, K % 64 == 0.
void launch_moe_gemm_fp8_bwd(int stage, const void* A, const int* offsets, const void* W, const float* kscale,
                             const float* nscale, const void* gu, void* out, int P, int E, int N, int K,
                             hipStream_t st) {
  const int nblk = (N + MG_BN - 1) / MG_BN;
  const int tiles = P < P / MG_BM + E ? P : P / MG_BM + E;
  const int grid = tiles * nblk;
  if (stage == 0)
    moe_gemm_nn_fp8_k<true><<<grid, 256, 0, st>>>((const bf16*)A, offsets, (const uint8_t*)W, kscale, nscale,
                                                  (const bf16*)gu, (bf16*)out, E, N, K, nblk);
  else
    moe_gemm_nn_fp8_k<false><<<grid, 256, 0, st>>>((const bf16*)A, offsets, (const uint8_t*)W, nullptr, nullptr,
                                                   nullptr, (bf16*)out, E, N, K, nblk);
  LIPA_CHECK_LAUNCH();
}
