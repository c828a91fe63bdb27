// FP8 (OCP e4m3) KV cache for serving (README §4, K23): the cache holds one byte per element and one fp32 scale
// per (token, kv-head) vector, quantised by quant/fp8.py::quantize_rows_reference with one row = one head vector:
//     amax = max(|x|, 2^-20), scale = amax / 448, codes = e4m3_rne(clamp(x · 448/amax, ±448)).
// Layout: k[layer], v[layer] are uint8 [B, Smax, Hkv·(D+16)]; a head block is D code bytes followed by a 16-byte
// tail whose first 4 bytes are the fp32 scale and whose other 12 are zero.  144 (D = 128) and 80 (D = 64) bytes
// keep every head block 16-byte aligned, and the scale travels with its codes through every row copy.
//
//  * decode_attn_fp8_k<D>: split-K decode attention over the codes with the append fused, grid (splits, Hkv, B),
//    4 waves, a wave owns 32-key tiles of its split.  Scores are computed swapped, Sᵀ = K·Qᵀ, with the G <= 16
//    query heads of the kv head as the MFMA columns.  A key's head block is D bytes, so the four lanes of a key
//    (li = key, g = lane >> 4) read 64 contiguous bytes, 16 codes each: ONE 16-byte load feeds TWO 32-deep K steps
//    (codes 0..7 of the load are step 2j's 8 k-values of lane group g, codes 8..15 step 2j+1's), and Q is loaded
//    once per workgroup with the same k order (d = 64j + 16g + 8h + i), which is all a dot product needs.
//    The codes are converted in registers, exactly (v_cvt_pk_f32_fp8, then bf16: e4m3 has 3 mantissa bits), and
//    multiplied by v_mfma_f32_16x16x32_bf16.  The K scale multiplies the fp32 score of its key together with
//    scale·log2(e); the V scale multiplies P before P is rounded to bf16, so V stays codes-as-bf16 through the
//    wave-private LDS tile and the transposed read ds_read_b64_tr_b16, and Oᵀ = Vᵀ·Pᵀ needs no rescale.  The 64
//    scales of a tile (32 K, 32 V) are ONE dword load per lane, handed round through 256 bytes of LDS per wave
//    and read back as the four consecutive keys a lane owns (ds_read_b128).
//    The split that holds the last key quantises the new token's K and V head vectors (wave 0 / wave 1, 16
//    elements per lane, amax by xor shuffles over the head's lanes), stores codes and tail into the cache at pos
//    and keeps the same 2·(D+16) bytes in LDS, where the tile that contains pos takes them from: the step uses
//    the bits every later step will read, and no workgroup reads cache[pos] in the launch that writes it.
//    Lengths come from pos (int64) on the device; the split count depends on (B, Hkv, max_len) alone.
//  * kv_fp8_write_rows_k<D>: prefill K and V rows [T, Hkv·D] bf16 (row-strided) → head blocks at cache row idx[t];
//    one lane per 16 elements, one 16-byte store per lane and one per tail.
//  * kv_fp8_dequant_rows_k<D>: cache rows → bf16 [n, Hkv·D] = bf16(code · scale): the op behind kv_fp8_dequant_rows.  No
//    serving path uses it since attn_prefill_fp8_k reads the codes; the benchmark's old path and the tests do.
//  * attn_prefill_fp8_k<D>: causal GQA flash-attention forward for prefill, chunked prefill, prefix hits and packed
//    admissions, reading the codes in place; grid (128-query block, q head, sequence) in xcd_grid3 order (the blocks
//    and then the heads of a GQA group are neighbours on one XCD and share the codes in its L2), sequences described
//    on the device by cu_q / slots / q_offs / kv_lens.  A 64-key tile is converted ONCE per workgroup: 16-byte
//    global loads of the codes into registers one tile ahead of the MFMAs, cvt16 (exact), and a bf16 image in
//    double-buffered LDS with D + 16 padded rows (the 16x16x32 K fragment reads ds_read_b128 and the transposed V
//    reads ds_read_b64_tr_b16 are both conflict-free at that stride), which all four waves read; the tile's 128
//    scales go through a small fp32 LDS array.  LDS-DMA moves bytes and cannot convert, so unlike attn_fwd128_k
//    this kernel stages through registers.  Scores are swapped (Sᵀ = K·Qᵀ, a lane owns a query, lane-local fp32
//    online softmax); as in the decode kernel the K scale multiplies the fp32 score with scale·log2(e) and the V
//    scale multiplies P before P is rounded to bf16.  Tiles are aligned to key 0 and visited in ascending order,
//    rows past the block's last visible row are never addressed, and skipped or masked tiles add exact zeros, so
//    a query's output bits depend on its q row, its position and the cache rows it sees alone.
#include "common.h"

using namespace lipa;

int decode_split_plan2(int B, int hkv, int max_len);   // decode.hip: the split count of the MFMA decode kernels

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr float E4M3_MAX = 448.f;
constexpr float AMAX_FLOOR = 0x1p-20f;

__device__ __forceinline__ bf16x4 tr_read(const bf16* p) {
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p));
}
__device__ __forceinline__ int split_chunk32(int len, int nsplit) { return ((len + nsplit - 1) / nsplit + 31) & ~31; }

// 16 e4m3 codes → 2 × 8 bf16, exact
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

// 16 bf16 of a head vector in this lane; amax over the head's D/16 lanes (a 16-lane aligned group at most)
__device__ __forceinline__ void load16(const bf16* p, float (&x)[16]) {
  const bf16x8 a = *reinterpret_cast<const bf16x8*>(p), b = *reinterpret_cast<const bf16x8*>(p + 8);
#pragma unroll
  for (int i = 0; i < 8; ++i) { x[i] = (float)a[i]; x[8 + i] = (float)b[i]; }
}
template <int LANES>
__device__ __forceinline__ float head_amax(const float (&x)[16]) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(x[i]));
#pragma unroll
  for (int o = 1; o < LANES; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  return fmaxf(amax, AMAX_FLOOR);
}
__device__ __forceinline__ u32x4 quant16(const float (&x)[16], float amax) {
  const float inv = E4M3_MAX / amax;
  u32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = fminf(fmaxf(x[4 * j + i] * inv, -E4M3_MAX), E4M3_MAX);
    uint32_t p = 0;
    p = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], p, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], p, true);
    o[j] = p;
  }
  return o;
}
__device__ __forceinline__ u32x4 tail16(float amax) { return u32x4{__float_as_uint(amax / E4M3_MAX), 0u, 0u, 0u}; }

// ============================================================================ decode attention + append
template <int D>
__global__ __launch_bounds__(256) void decode_attn_fp8_k(const bf16* __restrict__ q, int ldq,
                                                         const bf16* __restrict__ knew, int ldkn,
                                                         const bf16* __restrict__ vnew, int ldvn,
                                                         uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                         const int64_t* __restrict__ pos, float* __restrict__ opart,
                                                         float* __restrict__ mpart, float* __restrict__ lpart,
                                                         int Smax, int hq, int hkv, int nsplit, float scale_log2) {
  constexpr int HB = D + 16;          // bytes of a head block
  constexpr int HL = D / 16;          // lanes of a head vector at 16 elements each
  constexpr int LDR = D + 8;          // padded LDS row of the V tile (bf16 elements)
  constexpr int KL = D / 64;          // 16-byte K loads per lane and key, two K steps each
  constexpr int NS = D / 32;          // K steps over the head dim
  constexpr int ND = D / 16;          // d-subtiles of O
  constexpr int VL = 32 * HL / 64;    // 16-byte V loads per lane and 32-key tile
  constexpr int VT = 32 * LDR;        // elements of one wave's V tile
  __shared__ __attribute__((aligned(16))) char smem[4 * VT * 2];
  __shared__ __attribute__((aligned(16))) uint8_t snew[2][HB];     // the new token's K and V head blocks
  __shared__ __attribute__((aligned(16))) float sscl[4][64];       // per wave: 32 K scales, 32 V scales of a tile
  __shared__ float sm[4][16], sl[4][16];
  static_assert(4 * 16 * D * 4 <= 4 * VT * 2, "merge buffer aliases the V tiles");

  const int split = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
  const int G = hq / hkv;
  const int len = (int)pos[b] + 1;
  const int chunk = split_chunk32(len, nsplit);
  const int k0 = split * chunk, k1 = min(k0 + chunk, len);
  if (k0 >= len || len > Smax) return;   // whole workgroup: empty split, never merged (or a position outside the cache)
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;

  const size_t rs = (size_t)hkv * HB;
  uint8_t* kcb = kc + (size_t)b * Smax * rs + kh * HB;
  uint8_t* vcb = vc + (size_t)b * Smax * rs + kh * HB;
  const bool last = k1 == len;        // this split holds the new token (uniform over the workgroup)
  if (last) {
    if (w < 2) {                      // wave 0: K, wave 1: V; lanes 0..HL-1 the codes, lane HL the tail
      const bf16* src = (w == 0 ? knew + (size_t)b * ldkn : vnew + (size_t)b * ldvn) + kh * D;
      uint8_t* dst = (w == 0 ? kcb : vcb) + (size_t)(len - 1) * rs;
      float x[16];
      if (lane < HL) {
        load16(src + 16 * lane, x);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) x[i] = 0.f;
      }
      const float amax = head_amax<16>(x);         // whole wave shuffles; lanes 0..HL (<= 8) share a 16-lane group
      if (lane <= HL) {
        const u32x4 o = lane < HL ? quant16(x, amax) : tail16(amax);
        *reinterpret_cast<u32x4*>(&snew[w][16 * lane]) = o;
        *reinterpret_cast<u32x4*>(dst + 16 * lane) = o;
      }
    }
    __syncthreads();
  }

  // Q in the K loads' k order: step 2j + h holds d = 64j + 16g + 8h .. + 7
  bf16x8 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (li < G) qf[s] = *reinterpret_cast<const bf16x8*>(q + (size_t)b * ldq + (kh * G + li) * D + 64 * (s >> 1) + 16 * g + 8 * (s & 1));
    else qf[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  f32x4 acc[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  bf16* vl = reinterpret_cast<bf16*>(smem) + w * VT;
  float* scl = sscl[w];

  for (int t = k0 + 32 * w; t < k1; t += 128) {
    const bool fresh = last && t + 32 >= len;      // the tile that contains pos (uniform over the wave)
    u32x4 kr[2][KL], vr[VL];
    float sc1;
    if (!fresh) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const uint8_t* kp = kcb + (size_t)min(t + 16 * kt + li, k1 - 1) * rs + 16 * g;
#pragma unroll
        for (int j = 0; j < KL; ++j) kr[kt][j] = *reinterpret_cast<const u32x4*>(kp + 64 * j);
      }
#pragma unroll
      for (int p = 0; p < VL; ++p) {
        const int ci = p * 64 + lane, row = ci / HL, ch = ci % HL;
        vr[p] = *reinterpret_cast<const u32x4*>(vcb + (size_t)min(t + row, k1 - 1) * rs + 16 * ch);
      }
      sc1 = *reinterpret_cast<const float*>((lane < 32 ? kcb : vcb) + (size_t)min(t + (lane & 31), k1 - 1) * rs + D);
    } else {                                       // as above, with key len - 1 taken from LDS
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const int key = min(t + 16 * kt + li, k1 - 1);
        const uint8_t* kp = kcb + (size_t)key * rs + 16 * g;
#pragma unroll
        for (int j = 0; j < KL; ++j) {
          if (key == len - 1) kr[kt][j] = *reinterpret_cast<const u32x4*>(&snew[0][16 * g + 64 * j]);
          else kr[kt][j] = *reinterpret_cast<const u32x4*>(kp + 64 * j);
        }
      }
#pragma unroll
      for (int p = 0; p < VL; ++p) {
        const int ci = p * 64 + lane, row = ci / HL, ch = ci % HL;
        const int key = min(t + row, k1 - 1);
        if (key == len - 1) vr[p] = *reinterpret_cast<const u32x4*>(&snew[1][16 * ch]);
        else vr[p] = *reinterpret_cast<const u32x4*>(vcb + (size_t)key * rs + 16 * ch);
      }
      const int key = min(t + (lane & 31), k1 - 1);
      if (key == len - 1) sc1 = *reinterpret_cast<const float*>(&snew[lane >> 5][D]);
      else sc1 = *reinterpret_cast<const float*>((lane < 32 ? kcb : vcb) + (size_t)key * rs + D);
    }
    f32x4 sc[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < KL; ++j) {
        bf16x8 a0, a1;
        cvt16(kr[kt][j], a0, a1);
        sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, qf[2 * j], sc[kt], 0, 0, 0);
        sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, qf[2 * j + 1], sc[kt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int p = 0; p < VL; ++p) {
      const int ci = p * 64 + lane, row = ci / HL, ch = ci % HL;
      bf16x8 a0, a1;
      cvt16(vr[p], a0, a1);
      *reinterpret_cast<bf16x8*>(vl + row * LDR + 16 * ch) = a0;
      *reinterpret_cast<bf16x8*>(vl + row * LDR + 16 * ch + 8) = a1;
    }
    scl[lane] = sc1;
    __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): this wave's V tile and scales are in LDS
    __builtin_amdgcn_wave_barrier();
    // lane owns head li; keys t + 16kt + 4g + r
    f32x4 sk[2], sv[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      sk[kt] = *reinterpret_cast<const f32x4*>(scl + 16 * kt + 4 * g);
      sv[kt] = *reinterpret_cast<const f32x4*>(scl + 32 + 16 * kt + 4 * g);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = (t + 16 * kt + 4 * g + r < k1) ? sc[kt][r] * (sk[kt][r] * scale_log2) : -INFINITY;
        sc[kt][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m_run, mx);            // finite: every tile has >= 1 valid key
    const float alpha = __builtin_amdgcn_exp2f(m_run - mn);
    float rsum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = __builtin_amdgcn_exp2f(sc[kt][r] - mn);
        sc[kt][r] = pr * sv[kt][r];              // the V scale rides on P; the sum keeps the plain p
        rsum += pr;
      }
    rsum += __shfl_xor(rsum, 16, 64);
    rsum += __shfl_xor(rsum, 32, 64);
    l_run = l_run * alpha + rsum;
    m_run = mn;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) acc[dt] *= alpha;
    const bf16x8 pf = bf16x8{(bf16)sc[0][0], (bf16)sc[0][1], (bf16)sc[0][2], (bf16)sc[0][3],
                             (bf16)sc[1][0], (bf16)sc[1][1], (bf16)sc[1][2], (bf16)sc[1][3]};
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      const bf16* p0 = vl + (4 * g + (li >> 2)) * LDR + 16 * dt + 4 * (li & 3);
      const bf16x4 a = tr_read(p0), c = tr_read(p0 + 16 * LDR);
      const bf16x8 vf = bf16x8{a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
      acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[dt], 0, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);          // LDS reads done before the tile and the scales are rewritten
    __builtin_amdgcn_wave_barrier();
  }
  // ---- merge the 4 waves (Oᵀ[16dt + 4g + r][li]) through LDS, natural-log m for the merge kernel
  __syncthreads();
  float* sacc = reinterpret_cast<float*>(smem);   // [4][16][D], aliases the V tiles
  if (g == 0) {
    sm[w][li] = m_run;
    sl[w][li] = l_run;
  }
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) sacc[(w * 16 + li) * D + 16 * dt + 4 * g + r] = acc[dt][r];
  __syncthreads();
  for (int i = threadIdx.x; i < G * D; i += 256) {
    const int hh = i / D, d = i % D;
    const float M = fmaxf(fmaxf(sm[0][hh], sm[1][hh]), fmaxf(sm[2][hh], sm[3][hh]));
    float L = 0.f, A = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      const float c = __builtin_amdgcn_exp2f(sm[s2][hh] - M);   // -inf (idle wave) → 0
      L += sl[s2][hh] * c;
      A += sacc[(s2 * 16 + hh) * D + d] * c;
    }
    const size_t hrow = ((size_t)b * hq + kh * G + hh) * nsplit + split;
    opart[hrow * D + d] = A;
    if (d == 0) {
      mpart[hrow] = M * 0.6931471805599453f;
      lpart[hrow] = L;
    }
  }
}

template <int D>
__global__ __launch_bounds__(D) void decode_attn_fp8_merge_k(const float* __restrict__ opart,
                                                             const float* __restrict__ mpart,
                                                             const float* __restrict__ lpart,
                                                             const int64_t* __restrict__ pos, bf16* __restrict__ out,
                                                             int hq, int nsplit) {
  const size_t h = blockIdx.x;  // b*hq + head
  const int d = threadIdx.x;
  const int len = (int)pos[h / hq] + 1;
  const int chunk = max(split_chunk32(len, nsplit), 32);
  const int nv = len > 0 ? min(nsplit, (len + chunk - 1) / chunk) : 0;   // splits that wrote partials
  float M = -INFINITY;
  for (int s = 0; s < nv; ++s) M = fmaxf(M, mpart[h * nsplit + s]);
  float L = 0.f, A = 0.f;
  for (int s = 0; s < nv; ++s) {
    const float c = __expf(mpart[h * nsplit + s] - M);
    L += lpart[h * nsplit + s] * c;
    A += opart[(h * nsplit + s) * D + d] * c;
  }
  out[h * D + d] = (bf16)(L > 0.f ? A / L : 0.f);
}

// ============================================================================ prefill write
// K and V rows [T, Hkv·D] bf16 (row strides ldk / ldv elements) → head blocks at cache row idx[t] of kc / vc, seen
// as [R, Hkv·(D+16)].  blockIdx.y: 0 = K, 1 = V.  A thread owns 16 elements of one head vector; a row index outside
// [0, R) writes nothing.
template <int D>
__global__ __launch_bounds__(256) void kv_fp8_write_rows_k(const bf16* __restrict__ k, long ldk,
                                                           const bf16* __restrict__ v, long ldv,
                                                           uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                           const int64_t* __restrict__ idx, long T, int hkv, long R) {
  constexpr int HB = D + 16, HL = D / 16;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long head = gid / HL;         // t·Hkv + kh: the HL lanes of a head are an aligned group of one wave
  const int c = (int)(gid % HL);
  const bool on = head < T * hkv;
  const long t = on ? head / hkv : 0;
  const int kh = on ? (int)(head % hkv) : 0;
  const bf16* src = blockIdx.y == 0 ? k + t * ldk : v + t * ldv;
  float x[16];
  if (on) {
    load16(src + kh * D + 16 * c, x);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = 0.f;
  }
  const float amax = head_amax<HL>(x);
  const long row = on ? idx[t] : -1;
  if (row < 0 || row >= R) return;
  uint8_t* dst = (blockIdx.y == 0 ? kc : vc) + ((size_t)row * hkv + kh) * HB;
  *reinterpret_cast<u32x4*>(dst + 16 * c) = quant16(x, amax);
  if (c == 0) *reinterpret_cast<u32x4*>(dst + D) = tail16(amax);
}

// ============================================================================ dequant
// cache rows [n, Hkv·(D+16)] (row stride lds bytes) → bf16 [n, Hkv·D]; a thread owns 16 codes
template <int D>
__global__ __launch_bounds__(256) void kv_fp8_dequant_rows_k(const uint8_t* __restrict__ src, long lds,
                                                             bf16* __restrict__ out, long n, int hkv) {
  constexpr int HB = D + 16, HL = D / 16;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long head = gid / HL;
  const int c = (int)(gid % HL);
  if (head >= n * hkv) return;
  const long t = head / hkv;
  const int kh = (int)(head % hkv);
  const uint8_t* p = src + (size_t)t * lds + (size_t)kh * HB;
  const u32x4 codes = *reinterpret_cast<const u32x4*>(p + 16 * c);
  const float s = *reinterpret_cast<const float*>(p + D);
  bf16x8 o[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)codes[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)codes[i], true);
    o[i >> 1][4 * (i & 1)] = (bf16)(lo[0] * s);
    o[i >> 1][4 * (i & 1) + 1] = (bf16)(lo[1] * s);
    o[i >> 1][4 * (i & 1) + 2] = (bf16)(hi[0] * s);
    o[i >> 1][4 * (i & 1) + 3] = (bf16)(hi[1] * s);
  }
  bf16* dst = out + ((size_t)t * hkv + kh) * D + 16 * c;
  *reinterpret_cast<bf16x8*>(dst) = o[0];
  *reinterpret_cast<bf16x8*>(dst + 8) = o[1];
}

// ============================================================================ prefill attention over the codes
// Sequence b of the launch owns query rows cu_q[b] .. cu_q[b+1]-1 of q / out and cache slot slots[b]; query i sits
// at position q_offs[b] + i and sees rows j <= q_offs[b] + i (and j < kv_lens[b]) of its slot.  A workgroup is 128
// queries of one q head (4 waves × 2 subtiles of 16); key tiles are 64 rows, aligned to row 0, ascending, up to
// kend = the last row any query of the block sees: rows >= kend are never addressed (loads clamp to kend - 1, a
// visible row, and the mask drops the duplicates).
template <int D>
__global__ __launch_bounds__(256, 2) void attn_prefill_fp8_k(const bf16* __restrict__ Q, long ldq,
                                                             const uint8_t* __restrict__ kc,
                                                             const uint8_t* __restrict__ vc,
                                                             const int* __restrict__ cu_q, const int* __restrict__ slots,
                                                             const int* __restrict__ q_offs,
                                                             const int* __restrict__ kv_lens, bf16* __restrict__ O,
                                                             int T, int nslots, int Smax, int hq, int hkv,
                                                             float scale_log2) {
  constexpr int HB = D + 16;        // bytes of a head block
  constexpr int HL = D / 16;        // 16-code chunks of a head vector
  constexpr int LDR = D + 16;       // padded LDS row (bf16 elements): conflict-free for both fragment reads
  constexpr int TILE = 64 * LDR;    // elements of one K or V image
  constexpr int NS = D / 32;        // K steps over the head dim
  constexpr int ND = D / 16;        // d-subtiles of O
  constexpr int LOADS = 64 * HL / 256;
  constexpr int QT = 2, QB = 64 * QT;
  __shared__ __attribute__((aligned(16))) bf16 smem[4 * TILE];      // K0 V0 K1 V1
  __shared__ __attribute__((aligned(16))) float sscl[2][128];       // per buffer: 64 K scales, 64 V scales

  int i0, h, b;
  xcd_grid3(i0, h, b);
  const int qb = gridDim.x - 1 - i0;   // heavy (late) blocks first
  const int r0 = cu_q[b], Sq = cu_q[b + 1] - r0;
  if (qb * QB >= Sq) return;           // uniform: no query of this workgroup exists (or an empty sequence)
  const int slot = slots[b];
  if (slot < 0 || slot >= nslots || r0 < 0 || r0 + Sq > T) return;   // descriptors outside q or the cache
  const int hk = h / (hq / hkv);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
  const int qoff = q_offs[b];
  const int kvlen = min(kv_lens ? kv_lens[b] : Smax, Smax);
  const int kend = min(qoff + min(qb * QB + QB, Sq), kvlen);   // rows the block's last query sees
  const int nt = (kend + 63) / 64;
  const int q0 = qb * QB + 16 * QT * w;
  // last row any query of this wave sees; a wave with no query of its own computes nothing
  const int wlim = q0 < Sq ? min(qoff + min(q0 + 16 * QT, Sq) - 1, kvlen - 1) : -1;

  const size_t rs = (size_t)hkv * HB;
  const uint8_t* kcb = kc + (size_t)slot * Smax * rs + hk * HB;
  const uint8_t* vcb = vc + (size_t)slot * Smax * rs + hk * HB;

  // Q fragments (B operand of Sᵀ = K·Qᵀ): Q[q0 + 16qt + li][32s + 8g + j]; rows past Sq repeat the last query
  bf16x8 qf[QT][NS];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int qi = min(q0 + 16 * qt + li, Sq - 1);
#pragma unroll
    for (int s = 0; s < NS; ++s)
      qf[qt][s] = *reinterpret_cast<const bf16x8*>(Q + (size_t)(r0 + qi) * ldq + h * D + 32 * s + 8 * g);
  }
  f32x4 acc[ND][QT];
  float m_run[QT], l_run[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) acc[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
    m_run[qt] = -INFINITY;
    l_run[qt] = 0.f;
  }

  // a tile's codes (16 per load) and scales, in registers one tile ahead of the MFMAs
  u32x4 kr[LOADS], vr[LOADS];
  float scr = 0.f;
  auto load_tile = [&](int t) {
#pragma unroll
    for (int p = 0; p < LOADS; ++p) {
      const int ci = p * 256 + threadIdx.x;
      const size_t off = (size_t)min(t * 64 + ci / HL, kend - 1) * rs + 16 * (ci % HL);
      kr[p] = *reinterpret_cast<const u32x4*>(kcb + off);
      vr[p] = *reinterpret_cast<const u32x4*>(vcb + off);
    }
    if (threadIdx.x < 128)
      scr = *reinterpret_cast<const float*>((threadIdx.x < 64 ? kcb : vcb) + (size_t)min(t * 64 + lane, kend - 1) * rs + D);
  };
  // converted once for the four waves: codes → bf16 images (exact), scales → the fp32 array
  auto store_tile = [&](int buf) {
    bf16* Kl = smem + buf * 2 * TILE;
    bf16* Vl = Kl + TILE;
#pragma unroll
    for (int p = 0; p < LOADS; ++p) {
      const int ci = p * 256 + threadIdx.x;
      const int o = (ci / HL) * LDR + 16 * (ci % HL);
      bf16x8 a0, a1;
      cvt16(kr[p], a0, a1);
      *reinterpret_cast<bf16x8*>(Kl + o) = a0;
      *reinterpret_cast<bf16x8*>(Kl + o + 8) = a1;
      cvt16(vr[p], a0, a1);
      *reinterpret_cast<bf16x8*>(Vl + o) = a0;
      *reinterpret_cast<bf16x8*>(Vl + o + 8) = a1;
    }
    if (threadIdx.x < 128) sscl[buf][threadIdx.x] = scr;
  };

  if (nt > 0) load_tile(0);
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    store_tile(buf);
    __syncthreads();   // one barrier per tile: buffer buf was last read two tiles ago, before the previous barrier
    if (t + 1 < nt) load_tile(t + 1);
    const int k0 = t * 64;
    if (k0 > wlim) continue;   // wave-uniform: the tile lies above every query of this wave
    const bf16* Kl = smem + buf * 2 * TILE;
    const bf16* Vl = Kl + TILE;
    // ---- Sᵀ[key][q] for 4 key subtiles × QT query subtiles
    f32x4 sc[4][QT];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) sc[kt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Kl + (16 * kt + li) * LDR + 32 * s + 8 * g);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
          sc[kt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qt][s], sc[kt][qt], 0, 0, 0);
      }
    }
    // the lane's keys are k0 + 16kt + 4g + r: their K scales (with scale·log2e) and V scales
    f32x4 ks[4], sv[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      ks[kt] = *reinterpret_cast<const f32x4*>(&sscl[buf][16 * kt + 4 * g]) * scale_log2;
      sv[kt] = *reinterpret_cast<const f32x4*>(&sscl[buf][64 + 16 * kt + 4 * g]);
    }
    // ---- mask + online softmax in the log2 domain (lane owns query q0 + 16qt + li)
    bf16x8 pf[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      const int klim = min(qoff + min(q0 + 16 * qt + li, Sq - 1), kvlen - 1);   // last key this query sees
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = (k0 + 16 * kt + 4 * g + r <= klim) ? sc[kt][qt][r] * ks[kt][r] : -INFINITY;
          sc[kt][qt][r] = v;
          mx = fmaxf(mx, v);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m_run[qt], mx);
      const bool dead = mn == -INFINITY;   // no key seen yet (only with kv_lens < 1)
      const float alpha = dead ? 1.f : __builtin_amdgcn_exp2f(m_run[qt] - mn);
      float rsum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = dead ? 0.f : __builtin_amdgcn_exp2f(sc[kt][qt][r] - mn);
          sc[kt][qt][r] = pr * sv[kt][r];   // the V scale rides on P; the sum keeps the plain p
          rsum += pr;
        }
      rsum += __shfl_xor(rsum, 16, 64);
      rsum += __shfl_xor(rsum, 32, 64);
      l_run[qt] = l_run[qt] * alpha + rsum;
      m_run[qt] = mn;
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) acc[dt][qt] *= alpha;
      // P as B operand, permuted key order j ↔ 32kb + 16(j>>2) + 4g + (j&3)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
        pf[qt][kb] = bf16x8{(bf16)sc[2 * kb][qt][0], (bf16)sc[2 * kb][qt][1], (bf16)sc[2 * kb][qt][2],
                            (bf16)sc[2 * kb][qt][3], (bf16)sc[2 * kb + 1][qt][0], (bf16)sc[2 * kb + 1][qt][1],
                            (bf16)sc[2 * kb + 1][qt][2], (bf16)sc[2 * kb + 1][qt][3]};
    }
    // ---- Oᵀ[d][q] += Vᵀ[d][key] · Pᵀ[key][q]
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
        const bf16* p0 = Vl + (32 * kb + 4 * g + (li >> 2)) * LDR + 16 * dt + 4 * (li & 3);
        const bf16x4 a = tr_read(p0), c = tr_read(p0 + 16 * LDR);
        const bf16x8 vf = bf16x8{a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
          acc[dt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qt][kb], acc[dt][qt], 0, 0, 0);
      }
    }
  }
  // ---- epilogue: O[q][16dt + 4g + r] = acc / l
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int qi = q0 + 16 * qt + li;
    if (qi >= Sq) continue;
    const float inv = l_run[qt] > 0.f ? 1.f / l_run[qt] : 0.f;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (bf16)(acc[dt][qt][r] * inv);
      *reinterpret_cast<bf16x4*>(O + (size_t)(r0 + qi) * (hq * D) + h * D + 16 * dt + 4 * g) = o;
    }
  }
}

}  // namespace

void launch_prefill_attention_fp8(const void* q, long ldq, const void* kc, const void* vc, const int* cu_q,
                                  const int* slots, const int* q_offs, const int* kv_lens, void* out, int T, int N,
                                  int max_q, int nslots, int Smax, int hq, int hkv, int d, float scale, hipStream_t st) {
  if (N <= 0 || max_q <= 0) return;
  dim3 grid((max_q + 127) / 128, hq, N);
  const float sl2 = scale * 1.4426950408889634f;
  if (d == 128)
    attn_prefill_fp8_k<128><<<grid, 256, 0, st>>>((const bf16*)q, ldq, (const uint8_t*)kc, (const uint8_t*)vc, cu_q,
                                                  slots, q_offs, kv_lens, (bf16*)out, T, nslots, Smax, hq, hkv, sl2);
  else
    attn_prefill_fp8_k<64><<<grid, 256, 0, st>>>((const bf16*)q, ldq, (const uint8_t*)kc, (const uint8_t*)vc, cu_q,
                                                 slots, q_offs, kv_lens, (bf16*)out, T, nslots, Smax, hq, hkv, sl2);
  LIPA_CHECK_LAUNCH();
}

int decode_fp8_split_plan(int B, int hkv, int max_len) { return decode_split_plan2(B, hkv, max_len); }

void launch_decode_attention_fp8(const void* q, int ldq, const void* knew, int ldkn, const void* vnew, int ldvn,
                                 void* kc, void* vc, const int64_t* pos, float* opart, float* mpart, float* lpart,
                                 void* out, int B, int Smax, int hq, int hkv, int d, int nsplit, float scale,
                                 hipStream_t st) {
  dim3 grid(nsplit, hkv, B);
  const float sl2 = scale * 1.4426950408889634f;
#define P(D_)                                                                                                         \
  decode_attn_fp8_k<D_><<<grid, 256, 0, st>>>((const bf16*)q, ldq, (const bf16*)knew, ldkn, (const bf16*)vnew, ldvn, \
                                              (uint8_t*)kc, (uint8_t*)vc, pos, opart, mpart, lpart, Smax, hq, hkv,   \
                                              nsplit, sl2);                                                           \
  decode_attn_fp8_merge_k<D_><<<B * hq, D_, 0, st>>>(opart, mpart, lpart, pos, (bf16*)out, hq, nsplit)
  if (d == 128) { P(128); } else { P(64); }
#undef P
  LIPA_CHECK_LAUNCH();
}

void launch_kv_fp8_write_rows(const void* k, long ldk, const void* v, long ldv, void* kc, void* vc, const int64_t* idx,
                              long T, int hkv, int d, long R, hipStream_t st) {
  if (T <= 0) return;
  const long lanes = T * hkv * (d / 16);
  dim3 grid((unsigned)((lanes + 255) / 256), 2);
  if (d == 128)
    kv_fp8_write_rows_k<128><<<grid, 256, 0, st>>>((const bf16*)k, ldk, (const bf16*)v, ldv, (uint8_t*)kc, (uint8_t*)vc,
                                                   idx, T, hkv, R);
  else
    kv_fp8_write_rows_k<64><<<grid, 256, 0, st>>>((const bf16*)k, ldk, (const bf16*)v, ldv, (uint8_t*)kc, (uint8_t*)vc,
                                                  idx, T, hkv, R);
  LIPA_CHECK_LAUNCH();
}

void launch_kv_fp8_dequant_rows(const void* src, long lds, void* out, long n, int hkv, int d, hipStream_t st) {
  if (n <= 0) return;
  const long lanes = n * hkv * (d / 16);
  const unsigned grid = (unsigned)((lanes + 255) / 256);
  if (d == 128)
    kv_fp8_dequant_rows_k<128><<<grid, 256, 0, st>>>((const uint8_t*)src, lds, (bf16*)out, n, hkv);
  else
    kv_fp8_dequant_rows_k<64><<<grid, 256, 0, st>>>((const uint8_t*)src, lds, (bf16*)out, n, hkv);
  LIPA_CHECK_LAUNCH();
}
