// FP8 W8A8 linears for serving (README §4, K22; compressed-tensors FP8_DYNAMIC):
//     y[m, n] = (Σ_k xq[m, k]·wq[n, k]) · sx[m] · sw[n] (+ bias[n]) (+ residual[m, n])  → bf16, rounded once
// with xq, wq OCP e4m3 codes ([M, K] and [N, K], the checkpoint layout), sx one fp32 scale per token row
// (computed here, every step), sw one per output channel.  K % 128 == 0, N % 16 == 0.
//
// The codes stay e4m3 in HBM, L2 and LDS; the arithmetic is v_mfma_f32_16x16x32_f16 on codes converted in
// registers (v_cvt_pk_f32_fp8 + v_cvt_pkrtz_f16_f32: every e4m3 value is exact in fp16).  The FP8 matrix
// instructions were measured and are not used: v_mfma_f32_16x16x128_f8f6f4 and v_mfma_f32_16x16x32_fp8_fp8 (the
// same bits) align the products of a block to the largest one and truncate below a fixed width, which leaves
// the sum low by up to 2^-12 of that product — 4.13 times the per-element bound of tests/test_fp8_gpu.py on codes
// that span all of e4m3's exponents, where the fp16 instruction stays at 0.50 (a correctly rounded result).
// A K step is 128 bytes of 16 rows of each operand, 32 bytes per lane: lane (li = lane & 15, q = lane >> 4) holds
// row li, bytes 32q..32q+31 — 32 *contiguous* bytes of one row, for the weights and the activations alike, fed
// to four MFMAs 8 bytes at a time.  The instruction multiplies register slot s of lane group q of one operand
// with the same slot of the other, so with one address function for both operands every k meets its partner
// whatever order the hardware walks the slots in, and the four lanes of a row read one whole 128-byte line.
// That is why the [N, K] codes need no re-tiling at load.
//
// The weights are the MFMA's A operand and the tokens its B operand: a lane then owns 4 consecutive output
// channels n = 4q..4q+3 of token li, so scales, bias, residual and the bf16 result move as 8/16-byte vectors.
//
//  * fp8_quant_rows_k: one workgroup per row, the row held in registers (16 values per thread and pass) between
//    the amax reduction and the conversion — read once, 16-B loads and stores.  With SWIGLU the values are
//    bf16(silu(g)·u) of a [g | u] row, the bits swiglu_fwd_k would have stored.
//  * fp8_skinny_k (M <= 32, bound by the weight stream): a workgroup owns 32 output channels × a K slice; its
//    4 waves take the slice's 128-byte steps round-robin, every wave streaming its weights straight from HBM
//    into the A registers (UN steps × 2 tiles × 32 B per lane in flight) and the few token rows from L2 into
//    the B registers.  The 4 waves' accumulators meet in LDS and are summed in wave order; with more than one
//    K slice the fp32 partials [KS, M, N] go to fp8_splitk_reduce_k, which sums them in slice order.  The
//    slicing is a function of (N, K) alone and MFMA columns do not mix, so a token's output bits do not depend
//    on the batch it is in.  No atomics.
//  * fp8_tiled_k (M > 32): 32·WT × 32·WT output tile per workgroup (2 × 2 waves, WT × WT MFMA tiles each),
//    both code matrices staged per 128-byte K step through double-buffered LDS (global → registers one step
//    ahead → LDS; one barrier per step).  LDS rows are 128 B with the 16-B chunk index XOR-ed by (row >> 1) & 7,
//    which spreads the 16 rows of a ds_read_b128 group over all banks without padding.  No split-K.
#include "common.h"

using namespace lipa;

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr float E4M3_MAX = 448.f;
constexpr float AMAX_FLOOR = 0x1p-20f;

__device__ __forceinline__ float silu(float g) { return g / (1.f + __expf(-g)); }   // as elementwise.hip

__device__ __forceinline__ i32x8 mfma_zero() { return i32x8{0, 0, 0, 0, 0, 0, 0, 0}; }

#ifndef LIPA_FP8_MFMA
// One 128-byte K step of a 16-row operand as the lane holds it after conversion: 4 × 8 halves.  Every e4m3 value
// (2^-9 .. 448) is exact in fp16, so v_cvt_pk_f32_fp8 + v_cvt_pkrtz_f16_f32 lose nothing.
struct Op16 {
  f16x8 v[4];
};

__device__ __forceinline__ Op16 to_f16(i32x8 c) {
  Op16 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    u32x4 h;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(c[2 * j + d], false);
      const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(c[2 * j + d], true);
      h[2 * d] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(lo[0], lo[1]));
      h[2 * d + 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(hi[0], hi[1]));
    }
    o.v[j] = __builtin_bit_cast(f16x8, h);
  }
  return o;
}

// acc += A(16 × 128) · B(16 × 128)ᵀ; lane holds acc[A row 4q+e][B row li].  Four v_mfma_f32_16x16x32_f16: step j
// pairs bytes 8j..8j+7 of the two lanes' 32, the same bytes of both operands.
__device__ __forceinline__ f32x4 mfma_128(const Op16& a, const Op16& b, f32x4 acc) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.v[j], b.v[j], acc, 0, 0, 0);
  return acc;
}
#else
// A/B build (LIPA_HIP_DEFINES=-DLIPA_FP8_MFMA, never the default): the codes go to v_mfma_f32_16x16x128_f8f6f4 as
// they are.  It is kept so that the truncation that ruled this instruction out can be measured again with
// tests/test_fp8_gpu.py; the recorded run is profiles/r10/fp8_mfma_truncation.txt.
struct Op16 {
  i32x8 c;
};
__device__ __forceinline__ Op16 to_f16(i32x8 c) { return Op16{c}; }
__device__ __forceinline__ f32x4 mfma_128(const Op16& a, const Op16& b, f32x4 acc) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a.c, b.c, acc, 0, 0, 0, 0, 0, 0);
}
#endif

__device__ __forceinline__ i32x8 load32(const uint8_t* p) {
  const u32x4 lo = *reinterpret_cast<const u32x4*>(p), hi = *reinterpret_cast<const u32x4*>(p + 16);
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// 4 floats → 4 e4m3 bytes of clamp(v·inv, ±448), RNE
__device__ __forceinline__ uint32_t cvt4(const float* v, float inv) {
  float t[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = fminf(fmaxf(v[i] * inv, -E4M3_MAX), E4M3_MAX);
  uint32_t p = 0;
  p = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], p, false);
  p = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], p, true);
  return p;
}

// ============================================================================ row quantiser
// X [R, K] bf16 (SWIGLU: [R, 2K] = [g | u]) → codes [R, K], scale [R].  K % 16 == 0, K <= 4096·NP.
template <int NP, bool SWIGLU>
__global__ __launch_bounds__(256) void fp8_quant_rows_k(const bf16* __restrict__ X, size_t ldx,
                                                        uint8_t* __restrict__ codes, float* __restrict__ scale,
                                                        int K) {
  __shared__ float red[4];
  const size_t r = blockIdx.x;
  const bf16* xr = X + r * ldx;
  float v[NP][16];
  float amax = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int k = 16 * (threadIdx.x + 256 * p);
    if (k < K) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float a[8];
        load8(xr + k + 8 * h, a);
        if (SWIGLU) {
          float u[8];
          load8(xr + K + k + 8 * h, u);
#pragma unroll
          for (int i = 0; i < 8; ++i) a[i] = (float)(bf16)(silu(a[i]) * u[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          v[p][8 * h + i] = a[i];
          amax = fmaxf(amax, fabsf(a[i]));
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) v[p][i] = 0.f;
    }
  }
  amax = fmaxf(block_max<4>(amax, red), AMAX_FLOOR);
  const float inv = E4M3_MAX / amax;
  if (threadIdx.x == 0) scale[r] = amax / E4M3_MAX;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int k = 16 * (threadIdx.x + 256 * p);
    if (k < K) {
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = cvt4(&v[p][4 * j], inv);
      *reinterpret_cast<u32x4*>(codes + r * (size_t)K + k) = o;
    }
  }
}

// ============================================================================ epilogue
// 4 consecutive channels n..n+3 of token m
__device__ __forceinline__ void epilogue4(f32x4 s, const float* __restrict__ sx, const float* __restrict__ sw,
                                          const bf16* __restrict__ bias, const bf16* __restrict__ residual,
                                          bf16* __restrict__ out, size_t m, int n, int N) {
  const float xm = sx[m];
  const f32x4 w4 = *reinterpret_cast<const f32x4*>(sw + n);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = s[e] * xm * w4[e];
  if (bias) {
    const bf16x4 b = *reinterpret_cast<const bf16x4*>(bias + n);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += (float)b[e];
  }
  if (residual) {
    const bf16x4 rr = *reinterpret_cast<const bf16x4*>(residual + m * N + n);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += (float)rr[e];
  }
  const bf16x4 o = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  *reinterpret_cast<bf16x4*>(out + m * N + n) = o;
}

// ============================================================================ skinny GEMM, M <= 32
constexpr int SK_CT = 2;              // 16-channel MFMA tiles per workgroup (every wave takes both)
constexpr int SK_UN = 2;              // 128-byte K steps in flight per wave
constexpr int SK_MAX_M = 32;

template <int RT>
__global__ __launch_bounds__(256) void fp8_skinny_k(const uint8_t* __restrict__ XQ, const uint8_t* __restrict__ W,
                                                    const float* __restrict__ sx, const float* __restrict__ sw,
                                                    const bf16* __restrict__ bias, const bf16* __restrict__ residual,
                                                    bf16* __restrict__ out, float* __restrict__ part, int M, int N,
                                                    int K, int nct, int cpw) {
  __shared__ f32x4 red[4][SK_CT][RT][64];
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int cb = id % nct, ks = id / nct;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int nch = K / 128, c0 = ks * cpw, c1 = min(nch, c0 + cpw);
  const int n0 = cb * 16 * SK_CT;

  const uint8_t* wp[SK_CT];
#pragma unroll
  for (int ct = 0; ct < SK_CT; ++ct) wp[ct] = W + (size_t)min(n0 + 16 * ct + li, N - 1) * K + 32 * q;
  const uint8_t* xp[RT];
  bool xv[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    xv[rt] = 16 * rt + li < M;
    xp[rt] = XQ + (size_t)min(16 * rt + li, M - 1) * K + 32 * q;
  }

  f32x4 acc[SK_CT][RT];
#pragma unroll
  for (int ct = 0; ct < SK_CT; ++ct)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[ct][rt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c = c0 + w; c < c1; c += 4 * SK_UN) {       // the wave's steps: c0 + w, c0 + w + 4, ...
    i32x8 a[SK_UN][SK_CT], b[SK_UN][RT];
#pragma unroll
    for (int u = 0; u < SK_UN; ++u) {
      const int cc = c + 4 * u;
      if (cc < c1) {                                   // wave-uniform
#pragma unroll
        for (int ct = 0; ct < SK_CT; ++ct) a[u][ct] = load32(wp[ct] + (size_t)cc * 128);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) b[u][rt] = xv[rt] ? load32(xp[rt] + (size_t)cc * 128) : mfma_zero();
      }
    }
#pragma unroll
    for (int u = 0; u < SK_UN; ++u)
      if (c + 4 * u < c1) {
        Op16 ah[SK_CT], bh[RT];
#pragma unroll
        for (int ct = 0; ct < SK_CT; ++ct) ah[ct] = to_f16(a[u][ct]);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) bh[rt] = to_f16(b[u][rt]);
#pragma unroll
        for (int ct = 0; ct < SK_CT; ++ct)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[ct][rt] = mfma_128(ah[ct], bh[rt], acc[ct][rt]);
      }
  }

#pragma unroll
  for (int ct = 0; ct < SK_CT; ++ct)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) red[w][ct][rt][lane] = acc[ct][rt];
  __syncthreads();
  // wave j sums tile j = (ct, rt) over the 4 waves in wave order
  if (w < SK_CT * RT) {
    const int ct = w / RT, rt = w % RT;
    f32x4 s = red[0][ct][rt][lane];
#pragma unroll
    for (int j = 1; j < 4; ++j) s += red[j][ct][rt][lane];
    const int n = n0 + 16 * ct + 4 * q, m = 16 * rt + li;
    if (n < N && m < M) {
      if (part) *reinterpret_cast<f32x4*>(part + ((size_t)ks * M + m) * N + n) = s;
      else epilogue4(s, sx, sw, bias, residual, out, m, n, N);
    }
  }
}

// out[m, n..n+3] = epilogue(Σ_s part[s, m, n..n+3]) in slice order
__global__ __launch_bounds__(256) void fp8_splitk_reduce_k(const float* __restrict__ part, int KS,
                                                           const float* __restrict__ sx, const float* __restrict__ sw,
                                                           const bf16* __restrict__ bias,
                                                           const bf16* __restrict__ residual, bf16* __restrict__ out,
                                                           int M, int N) {
  const size_t MN = (size_t)M * N, i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(part + i);
  for (int k = 1; k < KS; ++k) s += *reinterpret_cast<const f32x4*>(part + (size_t)k * MN + i);
  epilogue4(s, sx, sw, bias, residual, out, i / N, (int)(i % N), N);
}

// ============================================================================ tiled GEMM, M > 32
__device__ __forceinline__ int swz(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

__device__ __forceinline__ i32x8 lds32(const uint8_t* t, int row, int q) {
  const u32x4 lo = *reinterpret_cast<const u32x4*>(t + swz(row, 2 * q));
  const u32x4 hi = *reinterpret_cast<const u32x4*>(t + swz(row, 2 * q + 1));
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

template <int WT>
__global__ __launch_bounds__(256) void fp8_tiled_k(const uint8_t* __restrict__ XQ, const uint8_t* __restrict__ W,
                                                   const float* __restrict__ sx, const float* __restrict__ sw,
                                                   const bf16* __restrict__ bias, const bf16* __restrict__ residual,
                                                   bf16* __restrict__ out, int M, int N, int K, int nbm) {
  constexpr int BT = 32 * WT;                      // tile rows of either operand; WT 16-B chunks per thread each
  __shared__ __attribute__((aligned(16))) uint8_t ws[2][BT * 128];
  __shared__ __attribute__((aligned(16))) uint8_t xs[2][BT * 128];
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int bm = id % nbm, bn = id / nbm;          // row blocks fastest: neighbours share the weight tile in L2
  const int m0 = bm * BT, n0 = bn * BT;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int wm = w & 1, wn = w >> 1;
  const int nkb = K / 128;

  u32x4 wr[WT], xr[WT];
  auto load_g = [&](int kb) {
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      const int idx = tid + 256 * j, row = idx >> 3, ch = idx & 7;
      const u32x4 z = {0u, 0u, 0u, 0u};
      wr[j] = n0 + row < N ? *reinterpret_cast<const u32x4*>(W + (size_t)(n0 + row) * K + (size_t)kb * 128 + 16 * ch) : z;
      xr[j] = m0 + row < M ? *reinterpret_cast<const u32x4*>(XQ + (size_t)(m0 + row) * K + (size_t)kb * 128 + 16 * ch) : z;
    }
  };
  auto store_s = [&](int buf) {
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      const int idx = tid + 256 * j, row = idx >> 3, ch = idx & 7;
      *reinterpret_cast<u32x4*>(ws[buf] + swz(row, ch)) = wr[j];
      *reinterpret_cast<u32x4*>(xs[buf] + swz(row, ch)) = xr[j];
    }
  };

  f32x4 acc[WT][WT];
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_g(0);
  store_s(0);
  __syncthreads();
  for (int kb = 0; kb < nkb; ++kb) {
    const int buf = kb & 1;
    if (kb + 1 < nkb) load_g(kb + 1);
    Op16 a[WT], b[WT];
#pragma unroll
    for (int i = 0; i < WT; ++i) a[i] = to_f16(lds32(ws[buf], 16 * (WT * wn + i) + li, q));
#pragma unroll
    for (int j = 0; j < WT; ++j) b[j] = to_f16(lds32(xs[buf], 16 * (WT * wm + j) + li, q));
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int j = 0; j < WT; ++j) acc[i][j] = mfma_128(a[i], b[j], acc[i][j]);
    if (kb + 1 < nkb) store_s(buf ^ 1);            // the buffer step kb-1 read; the barrier below closed those reads
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      const int n = n0 + 16 * (WT * wn + i) + 4 * q, m = m0 + 16 * (WT * wm + j) + li;
      if (n < N && m < M) epilogue4(acc[i][j], sx, sw, bias, residual, out, m, n, N);
    }
}

}  // namespace

void launch_fp8_quant_rows(const void* X, long ldx, void* codes, float* scale, int R, int K, bool swiglu,
                           hipStream_t st) {
  if (R <= 0) return;
#define L(NP_)                                                                                                    \
  do {                                                                                                            \
    if (swiglu) fp8_quant_rows_k<NP_, true><<<R, 256, 0, st>>>((const bf16*)X, (size_t)ldx, (uint8_t*)codes, scale, K); \
    else fp8_quant_rows_k<NP_, false><<<R, 256, 0, st>>>((const bf16*)X, (size_t)ldx, (uint8_t*)codes, scale, K);  \
  } while (0)
  if (K <= 4096) L(1); else if (K <= 8192) L(2); else L(4);
#undef L
  LIPA_CHECK_LAUNCH();
}

bool fp8_quant_supported(int K) { return K > 0 && K % 16 == 0 && K <= 16384; }

bool fp8_gemm_supported(int N, int K) { return N > 0 && K > 0 && N % 16 == 0 && K % 128 == 0; }

int fp8_skinny_max_m() { return SK_MAX_M; }

// 128-byte K steps per workgroup: the fewest slices (a multiple of 4 steps each, one per wave and round) that
// put >= 512 workgroups on the chip.  A function of (N, K) only — see the batch-invariance note on top.
int fp8_skinny_steps(int N, int K) {
  const int nct = (N + 16 * SK_CT - 1) / (16 * SK_CT), nch = K / 128;
  const int want = (512 + nct - 1) / nct;
  const int cpw = (nch + want - 1) / want;
  return cpw < 4 ? 4 : (cpw + 3) / 4 * 4;
}

int fp8_skinny_splits(int N, int K) {
  const int cpw = fp8_skinny_steps(N, K);
  return (K / 128 + cpw - 1) / cpw;
}

void launch_fp8_skinny(const void* xq, const void* w, const float* sx, const float* sw, const void* bias,
                       const void* res, void* out, float* part, int M, int N, int K, hipStream_t st) {
  const int nct = (N + 16 * SK_CT - 1) / (16 * SK_CT), cpw = fp8_skinny_steps(N, K), ks = fp8_skinny_splits(N, K);
  float* pp = ks > 1 ? part : nullptr;
  if (M <= 16)
    fp8_skinny_k<1><<<nct * ks, 256, 0, st>>>((const uint8_t*)xq, (const uint8_t*)w, sx, sw, (const bf16*)bias,
                                              (const bf16*)res, (bf16*)out, pp, M, N, K, nct, cpw);
  else
    fp8_skinny_k<2><<<nct * ks, 256, 0, st>>>((const uint8_t*)xq, (const uint8_t*)w, sx, sw, (const bf16*)bias,
                                              (const bf16*)res, (bf16*)out, pp, M, N, K, nct, cpw);
  if (ks > 1) {
    const size_t MN = (size_t)M * N;
    fp8_splitk_reduce_k<<<(unsigned)((MN / 4 + 255) / 256), 256, 0, st>>>(part, ks, sx, sw, (const bf16*)bias,
                                                                         (const bf16*)res, (bf16*)out, M, N);
  }
  LIPA_CHECK_LAUNCH();
}

// 64 × 64 tiles until 128 × 128 ones fill the 256 CUs (wt = 2 / 4 picks one; 0 = by shape)
void launch_fp8_tiled(const void* xq, const void* w, const float* sx, const float* sw, const void* bias,
                      const void* res, void* out, int M, int N, int K, int wt, hipStream_t st) {
  const long big = (long)((M + 127) / 128) * ((N + 127) / 128);
  if (wt == 4 || (wt == 0 && big >= 256)) {
    const int nbm = (M + 127) / 128;
    fp8_tiled_k<4><<<(unsigned)big, 256, 0, st>>>((const uint8_t*)xq, (const uint8_t*)w, sx, sw, (const bf16*)bias,
                                                  (const bf16*)res, (bf16*)out, M, N, K, nbm);
  } else {
    const int nbm = (M + 63) / 64, nbn = (N + 63) / 64;
    fp8_tiled_k<2><<<nbm * nbn, 256, 0, st>>>((const uint8_t*)xq, (const uint8_t*)w, sx, sw, (const bf16*)bias,
                                              (const bf16*)res, (bf16*)out, M, N, K, nbm);
  }
  LIPA_CHECK_LAUNCH();
}
