// Embedding pooling for gfx950: packed hidden states [T, H] (bf16 or fp32) -> unit vectors [N, dims] (fp32) in
// one launch: pick / average the rows of each sequence (cu_seqlens), keep the first `dims` columns (Matryoshka
// truncation: the other columns are never read), L2-normalise as F.normalize does.  ops/pooling.py::
// pool_embed_reference is the specification.
//
// Workgroup (s, b) = slice s of sequence b, 256 threads, every column of the row in one workgroup so the norm is
// one block reduction.  Threads are laid out as G row groups x CW 16-byte column chunks (CW = the chunk count
// rounded up to a power of two, at most 256; G = 256 / CW): a thread sums its chunk over rows g, g + G, ... of
// the slice in ascending order, the G partials are added in ascending g through LDS, rows wider than 256 chunks
// take several passes.  "last" and "cls" are the one-row case of the same code.
//
// A mean over more than POOL_SPLIT rows is cut into slices of POOL_SPLIT rows, one workgroup each (one 8k-token
// input alone would otherwise stream through a single CU).  Each slice stores its fp32 partial row; the slice
// that arrives last at the sequence's ticket counter adds the partials in ascending slice order and finishes the
// row.  No float atomics anywhere.  Slicing, thread layout and every summation order are functions of the
// sequence's own L and of dims alone: a sequence's vector has the same bits whatever else is in the pack and
// wherever it sits.
#include "common.h"

namespace lipa {

constexpr int POOL_SPLIT = 256;   // rows per workgroup of a mean-pooled sequence (ops/pooling.py::SPLIT_ROWS)
enum { POOL_LAST = 0, POOL_CLS = 1, POOL_MEAN = 2 };

template <typename T>
__global__ __launch_bounds__(256) void pool_embed_k(const T* __restrict__ hidden, long ldh,
                                                    const int* __restrict__ cu, float* __restrict__ out,
                                                    float* __restrict__ ws, int* __restrict__ cnt, int dims,
                                                    int mode, int normalize) {
  // [0, 2048): the row groups' partial chunks; [2048, 2052): block_sum scratch; [2052]: "this slice arrived last"
  __shared__ __attribute__((aligned(16))) float smem[2048 + 8];
  const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  const int a = cu[b], L = cu[b + 1] - a;
  const int nsplit = mode == POOL_MEAN ? max(1, (L + POOL_SPLIT - 1) / POOL_SPLIT) : 1;
  if (s >= nsplit) return;                      // uniform
  float* orow = out + (size_t)b * dims;
  if (L <= 0) {                                 // an empty sequence: a zero row, nothing read
    for (int c = tid; c < dims; c += 256) orow[c] = 0.f;
    return;
  }
  int r0 = 0, r1 = 1;                           // POOL_CLS
  if (mode == POOL_LAST) {
    r0 = L - 1;
    r1 = L;
  } else if (mode == POOL_MEAN) {
    r0 = s * POOL_SPLIT;
    r1 = min(L, r0 + POOL_SPLIT);
  }
  const float div = mode == POOL_MEAN ? (float)L : 1.f;
  const int nch = (dims + 7) >> 3;              // 16-B chunks (of 8 columns) that hold a kept column; 8·nch <= H
  int CW = 1;
  while (CW < nch && CW < 256) CW <<= 1;
  const int G = 256 / CW, cl = tid & (CW - 1), g = tid / CW;
  const T* base = hidden + (size_t)a * ldh;
  // slot of this sequence's slice s in the partial buffer: slices of different sequences never share one
  // (ceil(L / SPLIT) <= floor((a + L) / SPLIT) - floor(a / SPLIT) + 1)
  float* wrow = ws + ((size_t)(a / POOL_SPLIT) + b + s) * (size_t)(8 * nch);

  // y = pooled value of chunk c (divided, stored to the output row); returns its share of the squared norm
  auto emit = [&](int c, const float (&v)[8]) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int col = 8 * c + i;
      if (col < dims) {
        const float y = v[i] / div;
        orow[col] = y;
        ss = fmaf(y, y, ss);
      }
    }
    return ss;
  };
  // the row's norm over the block, then y / max(norm, 1e-12) on the values this thread stored itself
  auto finish = [&](float ss) {
    const float tot = block_sum<4>(ss, smem + 2048);
    if (!normalize) return;
    const float den = fmaxf(sqrtf(tot), 1e-12f);
    if (g == 0)
      for (int c = cl; c < nch; c += CW)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int col = 8 * c + i;
          if (col < dims) orow[col] = orow[col] / den;
        }
  };

  float ss = 0.f;
  for (int cb = 0; cb < nch; cb += CW) {
    const int c = cb + cl;
    const bool on = c < nch;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (on) {
      const T* p = base + 8 * c;
      int r = r0 + g;
      for (; r + 3 * G < r1; r += 4 * G) {      // four rows in flight, added in ascending row order
        float f0[8], f1[8], f2[8], f3[8];
        load8(p + (size_t)r * ldh, f0);
        load8(p + (size_t)(r + G) * ldh, f1);
        load8(p + (size_t)(r + 2 * G) * ldh, f2);
        load8(p + (size_t)(r + 3 * G) * ldh, f3);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = ((acc[i] + f0[i]) + f1[i]) + f2[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += f3[i];
      }
      for (; r < r1; r += G) {
        float f0[8];
        load8(p + (size_t)r * ldh, f0);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += f0[i];
      }
    }
    if (G > 1) {                                // add the row groups' partials in ascending g
      __syncthreads();
      store8(smem + 8 * tid, acc);              // 8·tid = (g·CW + cl)·8
      __syncthreads();
      if (g == 0) {
        for (int j = 1; j < G; ++j) {
          float f0[8];
          load8(smem + 8 * (j * CW + cl), f0);
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] += f0[i];
        }
      }
    }
    if (g == 0 && on) {
      if (nsplit == 1) ss += emit(c, acc);
      else store8(wrow + 8 * c, acc);
    }
  }
  if (nsplit == 1) {
    finish(ss);
    return;
  }

  // ---- sliced mean: publish this slice's partial row, draw a ticket; the last arriver adds the slices up.
  // plain stores -> every wave drains them -> barrier -> one agent-scope release -> ticket (relaxed, agent scope);
  // the last arriver: one agent-scope acquire -> barrier -> plain loads
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int ticket = __hip_atomic_fetch_add(cnt + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = ticket == nsplit - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    smem[2052] = last ? 1.f : 0.f;
  }
  __syncthreads();
  if (smem[2052] == 0.f) return;                // uniform
  const float* w0 = ws + ((size_t)(a / POOL_SPLIT) + b) * (size_t)(8 * nch);
  ss = 0.f;
  if (g == 0)
    for (int c = cl; c < nch; c += CW) {
      float acc[8];
      load8(w0 + 8 * c, acc);
      for (int j = 1; j < nsplit; ++j) {
        float f0[8];
        load8(w0 + (size_t)j * (8 * nch) + 8 * c, f0);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += f0[i];
      }
      ss += emit(c, acc);
    }
  finish(ss);
}

}  // namespace lipa

using namespace lipa;

int pool_embed_split_rows() { return POOL_SPLIT; }

// grid (max_nsplit, N): max_nsplit = slices of the longest mean-pooled sequence (1 for last / cls).  ws / cnt are
// needed (cnt zeroed) only when max_nsplit > 1: ws holds T / POOL_SPLIT + N + 1 rows of 8·ceil(dims / 8) floats.
void launch_pool_embed(const void* hidden, int is_f32, long ldh, const int* cu, float* out, float* ws, int* cnt,
                       int N, int dims, int mode, int normalize, int max_nsplit, hipStream_t st) {
  if (N <= 0) return;
  dim3 grid(max_nsplit, N), blk(256);
  if (is_f32)
    pool_embed_k<float><<<grid, blk, 0, st>>>((const float*)hidden, ldh, cu, out, ws, cnt, dims, mode, normalize);
  else
    pool_embed_k<bf16><<<grid, blk, 0, st>>>((const bf16*)hidden, ldh, cu, out, ws, cnt, dims, mode, normalize);
  LIPA_CHECK_LAUNCH();
}
