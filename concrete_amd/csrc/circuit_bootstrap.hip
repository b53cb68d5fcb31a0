// circuit_bootstrap.hip — the circuit bootstrap, stage 2 of the WoP-PBS, and the private functional packing
// keyswitch (fp-ks) it ends with (concrete-cuda cuda_circuit_bootstrap_64, cuda_fp_keyswitch_lwe_to_glwe_64,
// rust_api/src/cuda_bind.rs:334-364, 566-648).  All arithmetic mod 2^64.
//
// fp-ks key list: [k+1 keys][kN+1 blocks][l][(k+1)N] words; block j < kN belongs to bit j of the flattened GLWE
// key, block kN to the constant -1; storage index t of a block holds decomposition level l - t (the order of
// the LWE keyswitch keys, keyswitch.hip).  fp-ks of one LWE row x (kN + 1 words, body last) with key i:
//   out = - sum_{j = 0 .. kN} sum_level d_{j,level} key[i][j][level]
// with d the balanced signed decomposition of every word, the body included, and no body term added: the LWE
// keyswitch of the row (x, 0) with n_in = kN + 1 and n_out + 1 = (k+1)N, word for word.
//
// Circuit bootstrap of one LWE row c (n + 1 words) at delta_log; for v = 0 .. level_cbs-1, level = v + 1:
//   u = c * 2^(63 - delta_log), u.body += 2^62
//   w = PBS(u, acc_v), acc_v the trivial GLWE whose body coefficients all are -(2^(63 - base_log_cbs level))
//   w.body += 2^(63 - base_log_cbs level)
//   row i (0 .. k) of level matrix v of the output GGSW = fp-ks of w with key i
// Output per input: [level_cbs][k+1][(k+1)N], level matrix 0 = decomposition level 1: the order of one entry
// of a standard bootstrapping key and of concrete_hip_vertical_packing's ggsw_in (newer tfhe versions store
// GGSW levels reversed).
//
// One batched PBS over samples x level_cbs rows through the library's kernels (pbs_launch /
// pbs_generic_launch, gated as concrete_hip_pbs), small streams around it, then fpks_kernel, which writes
// GLWE (row, key) at row * (k+1) + key: the GGSW level matrices in place.  Nothing touches the host between
// the launches.
#include "../../include/concrete_hip.h"

#include <algorithm>
#include <type_traits>

#include "circuit_bootstrap.hpp"
#include "common.hpp"
#include "companion.hpp"
#include "pbs.hpp"

namespace chip {

// ------------------------------------------------------------------------------------------
// fp-ks.  Mostly wide digits (base_log 6 .. 24 at 8 .. 1 levels in the optimizer's WoP table; 8 of its 272
// rows, at (6, 7) and (8, 6), have digits as narrow as the int8 matrix-core keyswitch takes), a key of
// hundreds of MB and few rows: a workgroup keeps FPKS_ROWS rows x FPKS_THREADS columns of u64 sums in
// registers and streams its slice of the key once for all of them.
//
// Digits are stored offset, e = d + B/2 in [0, B] (B = 2^base_log): unsigned, so the low 64 bits of e * key
// are one 32 x 32 -> 64 multiply-add and one (DIG = uint32_t, base_log <= 31) or two (uint64_t) 32-bit
// products into a separate high-word sum; the offset comes back through the column sum of the key words,
// which costs one addition per key word:  - sum d key = (B/2) sum key - sum e key.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fpks_zero_kernel(uint64_t* __restrict__ out, uint64_t out_row_stride,
                                                        uint64_t per_row, uint64_t total) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const uint64_t r = e / per_row;
    out[r * out_row_stride + (e - r * per_row)] = 0ull;
  }
}

template <typename DIG>
__global__ void __launch_bounds__(FPKS_THREADS)
fpks_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ in, const uint64_t* __restrict__ key,
            uint64_t in_stride, uint64_t out_row_stride, uint32_t n_words, uint32_t G, uint32_t base_log,
            uint32_t level, uint32_t num_rows, uint32_t num_keys, uint32_t blocks_per_split) {
  __shared__ __attribute__((aligned(16))) DIG dig[FPKS_CHUNK][FPKS_ROWS];  // [(block, level) of the chunk][row]
  const uint32_t tid = threadIdx.x;
  const uint32_t col = blockIdx.x * FPKS_THREADS + tid;
  const uint32_t row0 = blockIdx.z * FPKS_ROWS;
  const uint32_t j_begin = blockIdx.y * blocks_per_split, j_end = min(n_words, j_begin + blocks_per_split);
  const uint32_t jch = (uint32_t)FPKS_CHUNK / level;  // blocks per chunk
  const int nrep = 64 - (int)(level * base_log);
  const uint64_t half = 1ull << (base_log - 1);
  const uint64_t key_words = (uint64_t)n_words * level * G;

  for (uint32_t j0 = j_begin; j0 < j_end; j0 += jch) {
    const uint32_t nj = min(jch, j_end - j0);
    __syncthreads();  // everyone is done with the previous chunk's digits
    for (uint32_t e = tid; e < FPKS_ROWS * nj; e += FPKS_THREADS) {
      const uint32_t r = e / nj, jj = e - r * nj;
      uint64_t a = 0ull;
      if (row0 + r < num_rows) a = in[(uint64_t)(row0 + r) * in_stride + j0 + jj];
      uint64_t st = decomp_init(a, nrep);
      for (uint32_t t = 0; t < level; ++t)
        dig[jj * level + t][r] = (DIG)((uint64_t)decomp_next64(st, (int)base_log) + half);
    }
    __syncthreads();
    if (col >= G) continue;  // (uniform per thread over the whole loop: it still reaches both barriers)
    const uint32_t nent = nj * level;
    for (uint32_t i = 0; i < num_keys; ++i) {
      uint64_t lo[FPKS_ROWS];
      uint32_t hi[FPKS_ROWS];
#pragma unroll
      for (int r = 0; r < FPKS_ROWS; ++r) lo[r] = 0ull, hi[r] = 0u;
      uint64_t ksum = 0ull;
      const uint64_t* kp = key + i * key_words + (uint64_t)j0 * level * G + col;
#pragma unroll 4
      for (uint32_t e = 0; e < nent; ++e) {
        const uint64_t kv = kp[(uint64_t)e * G];
        const uint32_t klo = (uint32_t)kv, khi = (uint32_t)(kv >> 32);
        ksum += kv;
#pragma unroll
        for (int r = 0; r < FPKS_ROWS; ++r) {
          const DIG d = dig[e][r];
          lo[r] += (uint64_t)(uint32_t)d * klo;
          if constexpr (std::is_same<DIG, uint32_t>::value) hi[r] += d * khi;
          else hi[r] += (uint32_t)d * khi + (uint32_t)(d >> 32) * klo;
        }
      }
      const uint64_t back = half * ksum;
#pragma unroll
      for (int r = 0; r < FPKS_ROWS; ++r) {
        if (row0 + r >= num_rows) break;
        const uint64_t v = back - (lo[r] + ((uint64_t)hi[r] << 32));
        atomicAdd((unsigned long long*)(out + (uint64_t)(row0 + r) * out_row_stride + (uint64_t)i * G + col),
                  (unsigned long long)v);
      }
    }
  }
}

bool fpks_params_ok(uint32_t k, uint32_t N, uint32_t level, uint32_t base_log) {
  const uint64_t n_words = (uint64_t)k * N + 1, G = ((uint64_t)k + 1) * N;
  if (k == 0 || N == 0 || n_words > 0xffffffffull || G > 0xffffffffull) return false;
  return keyswitch_params_ok(level, base_log, (uint32_t)n_words, (uint32_t)G - 1);
}

// Enough workgroups for the chip: the rows and the column windows first, then slices of the block axis, each
// of at least FPKS_MIN_BLOCKS blocks.
uint32_t fpks_splits(uint32_t n_words, uint32_t glwe_words, uint32_t num_rows) {
  const uint64_t wgs = (uint64_t)((glwe_words + FPKS_THREADS - 1) / FPKS_THREADS) *
                       ((num_rows + FPKS_ROWS - 1) / FPKS_ROWS);
  const uint64_t want = (FPKS_TARGET_WGS + wgs - 1) / wgs;
  const uint32_t most = std::max<uint32_t>(1, n_words / FPKS_MIN_BLOCKS);
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, most));
}

int fp_keyswitch_launch(const FpKsArgs& a) {
  if (a.num_rows == 0 || a.num_keys == 0) return 0;
  const uint64_t per_row = (uint64_t)a.num_keys * a.glwe_words, total = per_row * a.num_rows;
  hipLaunchKernelGGL(fpks_zero_kernel, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 4096)), dim3(256), 0,
                     a.stream, a.out, a.out_row_stride, per_row, total);
  uint32_t splits = fpks_splits(a.n_words, a.glwe_words, a.num_rows);
  const uint32_t per = (a.n_words + splits - 1) / splits;
  splits = (a.n_words + per - 1) / per;
  const dim3 grid((a.glwe_words + FPKS_THREADS - 1) / FPKS_THREADS, splits, (a.num_rows + FPKS_ROWS - 1) / FPKS_ROWS);
  // a balanced digit reaches +2^(base_log-1): offset by as much again it fits 32 bits up to base_log 31
  const auto kernel = a.base_log <= 31 ? fpks_kernel<uint32_t> : fpks_kernel<uint64_t>;
  hipLaunchKernelGGL(kernel, grid, dim3(FPKS_THREADS), 0, a.stream, a.out, a.in, a.key, a.in_stride, a.out_row_stride,
                     a.n_words, a.glwe_words, a.base_log, a.level, a.num_rows, a.num_keys, per);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  set_error("fp_keyswitch launch failed: %s", hipGetErrorString(e));
  return -1;
}

// ------------------------------------------------------------------------------------------
// the streams around the PBS
// ------------------------------------------------------------------------------------------
// PBS input row (s, v), for every v the same: input row s times 2^shift, 2^62 added to the body; and, when
// the call has no LUT index array of its own, the index v of the row's accumulator.
__global__ void __launch_bounds__(256) cbs_in_kernel(uint64_t* __restrict__ pbs_in, uint64_t* __restrict__ lut_idx,
                                                     const uint64_t* __restrict__ in, uint32_t shift,
                                                     uint32_t level_cbs, uint64_t w, uint64_t total) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const uint64_t r = e / w, c = e - r * w;
    uint64_t v = in[(r / level_cbs) * w + c] << shift;
    if (c == w - 1) v += 1ull << 62;
    pbs_in[e] = v;
    if (c == 0 && lut_idx) lut_idx[r] = r % level_cbs;
  }
}

// Accumulator v: k zero polynomials, then N coefficients -(2^(63 - base_log_cbs (v + 1))).
__global__ void __launch_bounds__(256) cbs_acc_kernel(uint64_t* __restrict__ acc, uint32_t base_log_cbs, uint64_t G,
                                                      uint64_t mask_len, uint64_t total) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const uint64_t v = e / G, j = e - v * G;
    acc[e] = j < mask_len ? 0ull : 0ull - (1ull << (63 - base_log_cbs * (uint32_t)(v + 1)));
  }
}

// The body constant of the PBS output rows: row r gets 2^(63 - base_log_cbs (v + 1)), v its LUT index.
__global__ void __launch_bounds__(256) cbs_body_kernel(uint64_t* __restrict__ pbs_out,
                                                       const uint64_t* __restrict__ lut_idx, uint32_t base_log_cbs,
                                                       uint64_t W, uint64_t rows) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  pbs_out[r * W + W - 1] += 1ull << ((63 - base_log_cbs * (uint32_t)(lut_idx[r] + 1)) & 63);
}

static uint32_t cbs_blocks(uint64_t threads) { return (uint32_t)std::min<uint64_t>((threads + 255) / 256, 256ull * 64); }

static uint64_t align16(uint64_t bytes) { return (bytes + 15) & ~15ull; }

static bool cbs_params_ok(uint32_t k, uint32_t N, uint32_t level_bsk, uint32_t base_log_bsk, uint32_t level_pksk,
                          uint32_t base_log_pksk, uint32_t level_cbs, uint32_t base_log_cbs) {
  const bool pbs = pbs_params_ok(k, N, level_bsk, base_log_bsk) || pbs_needs_generic_key(k, N, level_bsk, base_log_bsk);
  return pbs && fpks_params_ok(k, N, level_pksk, base_log_pksk) && level_cbs >= 1 &&
         (uint64_t)level_cbs * base_log_cbs <= 63;
}

// Scratch segments, each 16-byte aligned: PBS input (rows x (n+1)), PBS output (rows x (kN+1)), the level_cbs
// accumulators, the LUT indexes (rows); rows = samples x level_cbs.
struct CbsLayout {
  uint64_t pbs_in, pbs_out, acc, lut, bytes;
  bool ok;
};
static CbsLayout cbs_layout(uint32_t n, uint32_t k, uint32_t N, uint32_t level_cbs, uint32_t samples) {
  CbsLayout l{0, 0, 0, 0, 0, false};
  const uint64_t rows = (uint64_t)samples * level_cbs, G = ((uint64_t)k + 1) * N;
  // the PBS takes a 32-bit row count, the fp-ks one workgroup row (gridDim.z) per FPKS_ROWS rows
  if (rows == 0 || n == 0 || G == 0 || G > 65536 || rows > 65535ull * FPKS_ROWS) return l;
  const uint64_t W = (uint64_t)k * N + 1;
  l.pbs_in = 0;
  l.pbs_out = align16(8 * rows * ((uint64_t)n + 1));  // rows < 2^20, n + 1 <= 2^32: below 2^55
  l.acc = l.pbs_out + align16(8 * rows * W);
  l.lut = l.acc + align16(8 * G * level_cbs);
  l.bytes = l.lut + align16(8 * rows);
  l.ok = true;
  return l;
}

// The whole call.  lut_idx: the caller's LUT index array (the reference-named call), or nullptr.
static int cbs_run(void* stream, uint32_t gpu_index, uint64_t* ggsw_out, const uint64_t* lwe_in,
                   const void* fourier_bsk, const uint64_t* fp_ksk, const uint64_t* lut_idx, uint32_t delta_log,
                   uint32_t n, uint32_t k, uint32_t N, uint32_t level_bsk, uint32_t base_log_bsk, uint32_t level_pksk,
                   uint32_t base_log_pksk, uint32_t level_cbs, uint32_t base_log_cbs, uint32_t samples,
                   void* scratch, uint64_t scratch_bytes, uint64_t* pbs_out_copy) {
  // ---- validation: nothing below this block runs, and no HIP call is made, on a refused call ----
  if (samples == 0) return 0;
  if (!ggsw_out || !lwe_in || !fourier_bsk || !fp_ksk) {
    set_error("circuit_bootstrap: null pointer");
    return -1;
  }
  if (delta_log > 63) {
    set_error("circuit_bootstrap: delta_log=%u (at most 63)", delta_log);
    return -3;
  }
  if (!cbs_params_ok(k, N, level_bsk, base_log_bsk, level_pksk, base_log_pksk, level_cbs, base_log_cbs)) {
    set_error("circuit_bootstrap: unsupported parameters k=%u N=%u bsk level=%u base_log=%u, pksk level=%u "
              "base_log=%u, cbs level=%u base_log=%u",
              k, N, level_bsk, base_log_bsk, level_pksk, base_log_pksk, level_cbs, base_log_cbs);
    return -2;
  }
  const CbsLayout lay = cbs_layout(n, k, N, level_cbs, samples);
  if (!lay.ok) {
    set_error("circuit_bootstrap: lwe_dimension=%u num_samples=%u level_cbs=%u overflow the call's sizes", n, samples,
              level_cbs);
    return -3;
  }
  if (const int rc = scratch_refused("circuit_bootstrap", scratch, scratch_bytes, lay.bytes)) return rc;

  // ---- the key: concrete_hip_pbs's gates, refusing before anything is written ----
  PbsKey pk;
  if (const int rc = pbs_resolve_key(stream, gpu_index, fourier_bsk, n, k, N, base_log_bsk, level_bsk, &pk)) return rc;
  hipStream_t s = (hipStream_t)stream;

  const uint64_t rows = (uint64_t)samples * level_cbs, w = (uint64_t)n + 1, W = (uint64_t)k * N + 1;
  const uint64_t G = ((uint64_t)k + 1) * N;
  const CallScratch own(scratch, lay.bytes, s);
  char* base = own.base;
  uint64_t* d_pbs_in = (uint64_t*)(base + lay.pbs_in);
  uint64_t* d_pbs_out = (uint64_t*)(base + lay.pbs_out);
  uint64_t* d_acc = (uint64_t*)(base + lay.acc);
  uint64_t* d_lut = (uint64_t*)(base + lay.lut);

  hipLaunchKernelGGL(cbs_in_kernel, dim3(cbs_blocks(rows * w)), dim3(256), 0, s, d_pbs_in, lut_idx ? nullptr : d_lut,
                     lwe_in, 63 - delta_log, level_cbs, w, rows * w);
  hipLaunchKernelGGL(cbs_acc_kernel, dim3(cbs_blocks(G * level_cbs)), dim3(256), 0, s, d_acc, base_log_cbs, G,
                     (uint64_t)k * N, G * level_cbs);
  const uint64_t* lut = lut_idx ? lut_idx : d_lut;
  PbsArgs pa{s, d_pbs_out, nullptr, d_acc, lut, d_pbs_in, nullptr, pk.key, n, k, N, base_log_bsk, level_bsk, pk.limbs,
             (uint32_t)rows, nullptr, sync_guard((int)gpu_index, s)};
  int rc = pk.generic ? pbs_generic_launch(pa) : pbs_launch(pa);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(cbs_body_kernel, dim3(cbs_blocks(rows)), dim3(256), 0, s, d_pbs_out, lut, base_log_cbs, W, rows);
  if (pbs_out_copy) CHIP_CHECK(hipMemcpyAsync(pbs_out_copy, d_pbs_out, 8 * rows * W, hipMemcpyDeviceToDevice, s));
  const FpKsArgs fa{s, ggsw_out, d_pbs_out, fp_ksk, W, (k + 1) * G, (uint32_t)W, (uint32_t)G, base_log_pksk,
                    level_pksk, (uint32_t)rows, k + 1};
  rc = fp_keyswitch_launch(fa);
  const hipError_t e = hipGetLastError();
  if (rc == 0 && e != hipSuccess) {
    set_error("circuit_bootstrap launch failed: %s", hipGetErrorString(e));
    rc = -1;
  }
  return rc;
}

static ScratchRegistry g_cbs_scratch;  // the buffers handed out by scratch_cuda_circuit_bootstrap_64

}  // namespace chip

using namespace chip;

extern "C" {

uint64_t concrete_hip_fpksk_size_words(uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_count) {
  typedef unsigned __int128 u128;
  const u128 words = (u128)(glwe_dimension + 1ull) * ((u128)glwe_dimension * polynomial_size + 1) * level_count *
                     ((u128)(glwe_dimension + 1ull) * polynomial_size);
  return words >> 64 ? 0 : (uint64_t)words;
}

int concrete_hip_fp_keyswitch(void* stream, uint32_t gpu_index, uint64_t* glwe_array_out, const uint64_t* lwe_array_in,
                              const uint64_t* fp_ksk, uint32_t lwe_dimension_in, uint32_t glwe_dimension,
                              uint32_t polynomial_size, uint32_t base_log, uint32_t level_count, uint32_t num_rows,
                              uint32_t num_keys) {
  if (num_rows == 0) return 0;
  if (!glwe_array_out || !lwe_array_in || !fp_ksk) {
    set_error("fp_keyswitch: null pointer");
    return -1;
  }
  if (num_keys == 0 || (uint64_t)glwe_dimension * polynomial_size != lwe_dimension_in) {
    set_error("fp_keyswitch: num_keys=%u must be positive and lwe_dimension_in=%u must be glwe_dimension * "
              "polynomial_size = %u * %u",
              num_keys, lwe_dimension_in, glwe_dimension, polynomial_size);
    return -3;
  }
  if (!fpks_params_ok(glwe_dimension, polynomial_size, level_count, base_log)) {
    set_error("fp_keyswitch: unsupported parameters k=%u N=%u level=%u base_log=%u", glwe_dimension, polynomial_size,
              level_count, base_log);
    return -2;
  }
  const uint64_t G = ((uint64_t)glwe_dimension + 1) * polynomial_size;
  typedef unsigned __int128 u128;
  if (num_rows > 65535ull * FPKS_ROWS || ((u128)num_rows * num_keys * G * 8) >> 62 ||
      ((u128)num_keys * (lwe_dimension_in + 1ull) * level_count * G * 8) >> 62) {
    set_error("fp_keyswitch: num_rows=%u num_keys=%u overflow the call's sizes", num_rows, num_keys);
    return -3;
  }
  CHIP_CHECK(hipSetDevice((int)gpu_index));
  const FpKsArgs a{(hipStream_t)stream, glwe_array_out, lwe_array_in, fp_ksk, (uint64_t)lwe_dimension_in + 1,
                   num_keys * G, lwe_dimension_in + 1, (uint32_t)G, base_log, level_count, num_rows, num_keys};
  return fp_keyswitch_launch(a);
}

int concrete_hip_circuit_bootstrap_supported(uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_bsk,
                                             uint32_t base_log_bsk, uint32_t level_pksk, uint32_t base_log_pksk,
                                             uint32_t level_cbs, uint32_t base_log_cbs) {
  return cbs_params_ok(glwe_dimension, polynomial_size, level_bsk, base_log_bsk, level_pksk, base_log_pksk, level_cbs,
                       base_log_cbs)
             ? 1
             : 0;
}

uint64_t concrete_hip_circuit_bootstrap_scratch_bytes(uint32_t lwe_dimension, uint32_t glwe_dimension,
                                                      uint32_t polynomial_size, uint32_t level_cbs,
                                                      uint32_t num_samples) {
  const CbsLayout l = cbs_layout(lwe_dimension, glwe_dimension, polynomial_size, level_cbs, num_samples);
  return l.ok ? l.bytes : 0;
}

int concrete_hip_circuit_bootstrap(void* stream, uint32_t gpu_index, uint64_t* ggsw_out, const uint64_t* lwe_array_in,
                                   const void* fourier_bsk, const uint64_t* fp_ksk, uint32_t delta_log,
                                   uint32_t lwe_dimension, uint32_t glwe_dimension, uint32_t polynomial_size,
                                   uint32_t level_bsk, uint32_t base_log_bsk, uint32_t level_pksk,
                                   uint32_t base_log_pksk, uint32_t level_cbs, uint32_t base_log_cbs,
                                   uint32_t num_samples, void* scratch, uint64_t scratch_bytes, uint64_t* pbs_out) {
  return cbs_run(stream, gpu_index, ggsw_out, lwe_array_in, fourier_bsk, fp_ksk, nullptr, delta_log, lwe_dimension,
                 glwe_dimension, polynomial_size, level_bsk, base_log_bsk, level_pksk, base_log_pksk, level_cbs,
                 base_log_cbs, num_samples, scratch, scratch_bytes, pbs_out);
}

// Input row i goes through key i mod number_of_keys into GLWE i: per key q one launch on the rows q, q +
// number_of_keys, .. (strided rows in, strided GLWEs out).
void cuda_fp_keyswitch_lwe_to_glwe_64(void* stream, uint32_t gpu_index, void* glwe_array_out, const void* lwe_array_in,
                                      const void* fp_ksk_array, uint32_t input_lwe_dimension,
                                      uint32_t output_glwe_dimension, uint32_t output_polynomial_size,
                                      uint32_t base_log, uint32_t level_count, uint32_t number_of_input_lwe,
                                      uint32_t number_of_keys) {
  const char* what = "cuda_fp_keyswitch_lwe_to_glwe_64";
  if (number_of_input_lwe == 0) return;
  if (!glwe_array_out || !lwe_array_in || !fp_ksk_array) {
    set_error("null pointer");
    die(what);
  }
  const uint32_t k = output_glwe_dimension, N = output_polynomial_size;
  if (number_of_keys == 0 || (uint64_t)k * N != input_lwe_dimension || !fpks_params_ok(k, N, level_count, base_log) ||
      number_of_input_lwe > 65535u * FPKS_ROWS) {
    set_error("unsupported parameters: input_lwe_dimension=%u k=%u N=%u level=%u base_log=%u inputs=%u keys=%u",
              input_lwe_dimension, k, N, level_count, base_log, number_of_input_lwe, number_of_keys);
    die(what);
  }
  CHIP_CHECK(hipSetDevice((int)gpu_index));
  const uint64_t W = (uint64_t)input_lwe_dimension + 1, G = ((uint64_t)k + 1) * N;
  const uint64_t key_words = W * level_count * G;
  for (uint32_t q = 0; q < number_of_keys && q < number_of_input_lwe; ++q) {
    const uint32_t rows = (number_of_input_lwe - q + number_of_keys - 1) / number_of_keys;
    const FpKsArgs a{(hipStream_t)stream, (uint64_t*)glwe_array_out + q * G, (const uint64_t*)lwe_array_in + q * W,
                     (const uint64_t*)fp_ksk_array + q * key_words, number_of_keys * W, number_of_keys * G,
                     (uint32_t)W, (uint32_t)G, base_log, level_count, rows, 1};
    if (fp_keyswitch_launch(a) != 0) die(what);
  }
}

void scratch_cuda_circuit_bootstrap_64(void* stream, uint32_t gpu_index, int8_t** cbs_buffer, uint32_t glwe_dimension,
                                       uint32_t lwe_dimension, uint32_t polynomial_size, uint32_t level_count,
                                       uint32_t number_of_inputs, uint32_t max_shared_memory,
                                       bool allocate_gpu_memory) {
  (void)max_shared_memory;
  if (!cbs_buffer) {
    set_error("null buffer pointer");
    die("scratch_cuda_circuit_bootstrap_64");
  }
  *cbs_buffer = nullptr;
  const uint64_t bytes = concrete_hip_circuit_bootstrap_scratch_bytes(lwe_dimension, glwe_dimension, polynomial_size,
                                                                      level_count, number_of_inputs);
  if (!allocate_gpu_memory || bytes == 0) return;  // NULL: cuda_circuit_bootstrap_64 takes pool scratch
  *cbs_buffer = g_cbs_scratch.allocate(gpu_index, bytes, stream);
}

void cuda_circuit_bootstrap_64(void* stream, uint32_t gpu_index, void* ggsw_out, const void* lwe_array_in,
                               const void* fourier_bsk, const void* fp_ksk_array, const void* lut_vector_indexes,
                               int8_t* cbs_buffer, uint32_t delta_log, uint32_t polynomial_size,
                               uint32_t glwe_dimension, uint32_t lwe_dimension, uint32_t level_bsk,
                               uint32_t base_log_bsk, uint32_t level_pksk, uint32_t base_log_pksk, uint32_t level_cbs,
                               uint32_t base_log_cbs, uint32_t number_of_samples, uint32_t max_shared_memory) {
  (void)max_shared_memory;
  const char* what = "cuda_circuit_bootstrap_64";
  // a `dest` of cuda_convert_lwe_programmable_bootstrap_key_64 stands for its registered Fourier key;
  // any other pointer is a caller-owned Fourier key
  const void* f = concrete_hip_lookup_bsk(fourier_bsk);
  if (!f) f = fourier_bsk;
  const uint64_t bytes = g_cbs_scratch.size_of(what, "scratch_cuda_circuit_bootstrap_64", cbs_buffer);
  if (cbs_run(stream, gpu_index, (uint64_t*)ggsw_out, (const uint64_t*)lwe_array_in, f, (const uint64_t*)fp_ksk_array,
              (const uint64_t*)lut_vector_indexes, delta_log, lwe_dimension, glwe_dimension, polynomial_size,
              level_bsk, base_log_bsk, level_pksk, base_log_pksk, level_cbs, base_log_cbs, number_of_samples,
              cbs_buffer, bytes, nullptr) != 0)
    die(what);
}

void cleanup_cuda_circuit_bootstrap(void* stream, uint32_t gpu_index, int8_t** cbs_buffer) {
  g_cbs_scratch.release(gpu_index, cbs_buffer, stream);
}

}  // extern "C"
