// circuit_bootstrap.hpp — the private functional packing keyswitch (fp-ks) of the circuit bootstrap
// (circuit_bootstrap.hip): tile geometry and launch descriptor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chip {

// A workgroup of FPKS_THREADS threads owns FPKS_THREADS output columns (one per thread), FPKS_ROWS input
// rows and a slice of the key's (block, level) axis, which it walks in chunks of at most FPKS_CHUNK
// (block, level) entries: the chunk's digits of its rows sit in LDS, every key word of the chunk is read
// once and applied to all FPKS_ROWS rows.
constexpr int FPKS_THREADS = 256;
constexpr int FPKS_ROWS = 16;
constexpr int FPKS_CHUNK = 256;
// workgroups a launch aims for (eight per CU of 256) when it splits the (block, level) axis, and the fewest
// blocks a split keeps
constexpr uint32_t FPKS_TARGET_WGS = 2048;
constexpr uint32_t FPKS_MIN_BLOCKS = 16;

// out[(r, i)] = - sum_{j < n_words} sum_t d(in[r][j], t) key[i][j][t], rows r < num_rows, keys i < num_keys.
// Row r is read at in + r * in_stride; GLWE (r, i) is written at out + r * out_row_stride + i * glwe_words.
// The launch zeroes those outputs first: the workgroups add their partial sums atomically.
struct FpKsArgs {
  hipStream_t stream;
  uint64_t* out;
  const uint64_t* in;
  const uint64_t* key;       // [num_keys][n_words][level][glwe_words]
  uint64_t in_stride, out_row_stride;
  uint32_t n_words;          // kN + 1
  uint32_t glwe_words;       // (k+1) N
  uint32_t base_log, level, num_rows, num_keys;
};
// 0, or -1 with the message set; the caller has checked the parameters (fpks_params_ok)
int fp_keyswitch_launch(const FpKsArgs& a);
bool fpks_params_ok(uint32_t k, uint32_t N, uint32_t level, uint32_t base_log);
// slices of the (block, level) axis of a launch on num_rows rows (1: not split)
uint32_t fpks_splits(uint32_t n_words, uint32_t glwe_words, uint32_t num_rows);

}  // namespace chip
