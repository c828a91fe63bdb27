// Arguments of the per-row sampler (decode.hip sample_rows_k), shared with the binding.
#pragma once
#include <cstdint>

namespace lipa {

constexpr int SAMPLE_ROWS_MAX_BIAS = 300;   // logit_bias entries per row (the OpenAI API's limit)

struct SampleRows {
  const float* temperature;   // [B]; <= 0: greedy
  const int* top_k;           // [B]; <= 0 or >= V: off
  const float* top_p;         // [B]
  const float* min_p;         // [B]
  const float* rep;           // [B] repetition penalty (1 = off)
  const float* pres;          // [B] presence penalty (0 = off)
  const float* freq;          // [B] frequency penalty (0 = off)
  const int64_t* key;         // [B]; >= 0: the row's own key, < 0: derived from call_key and the row index
  const int* bias_id;         // [B, NB], -1 = unused
  const float* bias_val;      // [B, NB]
  int NB;
  const int* hist;            // [R, Lmax] or null
  const int* slot;            // [B] row -> history row
  const int* prompt_len;      // [B]
  const int* seq_len;         // [B]
  int R, Lmax;
  uint64_t call_key;
};

}  // namespace lipa
