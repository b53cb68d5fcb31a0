// vertical_packing.hip — vertical packing, stage 3 of the WoP-PBS (concrete-cuda cuda_cmux_tree_64 and
// cuda_blind_rotate_and_sample_extraction_64, rust_api/src/cuda_bind.rs:369-488).
//
// Per lookup, with cmux(c0, c1, G) = c0 + G [x] (c1 - c0) and [x] the exact external product of
// DESIGN.md §3 (all arithmetic mod 2^64):
//   tree      leaves = the trivial GLWEs of the 2^r LUT polynomials of an output; layer j = 0 .. r-1
//             uses tree GGSW r-1-j (the list is most significant bit first) and its node i is
//             cmux(prev[2i], prev[2i+1], G); one GLWE per output remains
//   rotation  for j = m-1 down to 0, d = 2^(m-1-j): acc = cmux(acc, X^(-d) acc, G_j)
//   extract   the sample extraction of the result, kN + 1 words
//
// The GGSWs exist only at run time, so each call converts them into the general key format
// (gen_convert_kernel, natural frequency order) and puts them through the per-key gate of §3.1: the
// conversion reduces max|G|, the host reads it (ONE stream synchronisation per call, as every key
// conversion costs) and the call returns -2, before anything is written, when the certified bound at
// that max|G| reaches 1/2.  After that the call is one gen_cmux_kernel launch (pbs_generic.hip) per tree
// layer and rotation step, layers alternating between two scratch buffers, and one extraction launch:
// no host synchronisation, no device-to-host copy and no allocation between them.
#include "../../include/concrete_hip.h"

#include <algorithm>

#include "common.hpp"
#include "companion.hpp"
#include "pbs.hpp"
#include "vertical_packing.hpp"

namespace chip {

constexpr uint32_t VP_MAX_R = 24;

// The first accumulators when no tree layer runs, one copy per lookup: per (lookup, output) the caller's GLWE
// (the two-call form's rotation), or the trivial GLWE of the output's LUT polynomial (r = 0;
// lut.hip's trivial_glwe_kernel writes one GLWE per LUT and has no lookup to repeat them over).  Word by
// word: the caller's buffers are only promised 8-byte alignment, and the stream is rows x (k+1) N words once
// per call.
__global__ void __launch_bounds__(256) vp_seed_kernel(uint64_t* __restrict__ dst, const uint64_t* __restrict__ glwes,
                                                      const uint64_t* __restrict__ luts, uint64_t G, uint64_t mask_len,
                                                      uint64_t per_lookup, uint64_t total) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const uint64_t j = e % G, o = (e / G) % per_lookup;
    dst[e] = glwes ? glwes[o * G + j] : j < mask_len ? 0ull : luts[o * (G - mask_len) + (j - mask_len)];
  }
}

static uint64_t align16(uint64_t bytes) { return (bytes + 15) & ~15ull; }

// Scratch segments, each 16-byte aligned: the converted GGSWs, then the two layer buffers.  Buffer A
// takes the layers 0, 2, ..: lookups x tau x 2^(r-1) GLWEs at most; buffer B the layers 1, 3, ..:
// lookups x tau x 2^(r-2).  Both hold at least lookups x tau GLWEs for the rotation.
struct VpLayout {
  uint64_t keys, a, b, bytes;
  bool ok;
};
static VpLayout vp_layout(uint32_t k, uint32_t N, uint32_t level, uint32_t r, uint32_t m, uint32_t tau,
                          uint32_t lookups) {
  VpLayout l{0, 0, 0, 0, false};
  const KeyFormat f = generic_key_format(k, N, level);
  if (f.kind != KeyKind::GENERIC || r > VP_MAX_R || tau == 0 || lookups == 0) return l;
  typedef unsigned __int128 u128;
  const u128 glwe = (u128)(k + 1) * N * 8;
  const u128 outs = (u128)lookups * tau;
  const u128 key_bytes = (u128)lookups * (r + m) * generic_fourier_bsk_bytes(1, k, level, N);
  const u128 a_bytes = outs * glwe << (r >= 1 ? r - 1 : 0), b_bytes = outs * glwe << (r >= 2 ? r - 2 : 0);
  const u128 total = key_bytes + a_bytes + b_bytes + 48;
  // every CMUX of a layer is a workgroup per output column, every standard polynomial of the GGSWs a
  // workgroup of the conversion: both grids must fit 31 bits
  const u128 conv_blocks = (u128)lookups * (r + m) * level * (k + 1) * (k + 1);
  if (total >> 62 || ((outs << (r >= 1 ? r - 1 : 0)) * (k + 1)) >> 31 || conv_blocks >> 31) return l;
  l.keys = 0;
  l.a = align16((uint64_t)key_bytes);
  l.b = l.a + align16((uint64_t)a_bytes);
  l.bytes = l.b + align16((uint64_t)b_bytes);
  l.ok = true;
  return l;
}

static uint32_t log2u(uint32_t N) { return 31u - (uint32_t)__builtin_clz(N); }

// The whole call.  glwe_in (the two-call form's rotation; needs r = 0): `tau` GLWEs that take the
// place of the tree's result, shared by the lookups.
static int vp_run(void* stream, uint32_t gpu_index, uint64_t* lwe_array_out, uint64_t* glwe_tree_out,
                  const uint64_t* ggsw_in, const uint64_t* lut_vector, const uint64_t* glwe_in, uint32_t k, uint32_t N,
                  uint32_t base_log, uint32_t level, uint32_t r, uint32_t m, uint32_t tau, uint32_t lookups,
                  void* scratch, uint64_t scratch_bytes, uint64_t* resid_bits, double* ggsw_spectrum_max) {
  // ---- validation: no HIP call is made on a refused call ----
  if ((!lut_vector && !glwe_in) || (!ggsw_in && r + m > 0)) {
    set_error("vertical_packing: null pointer");
    return -1;
  }
  if (tau == 0 || lookups == 0) {
    set_error("vertical_packing: tau=%u and num_lookups=%u must be positive", tau, lookups);
    return -3;
  }
  if (r > VP_MAX_R || N == 0 || m > log2u(N)) {
    set_error("vertical_packing: r=%u (at most %u), mbr_size=%u (at most log2 N, N=%u)", r, VP_MAX_R, m, N);
    return -3;
  }
  if (!lwe_array_out && (m > 0 || !glwe_tree_out)) {
    set_error("vertical_packing: lwe_array_out may be NULL only with mbr_size = 0 and glwe_tree_out given");
    return -3;
  }
  // vp_params_ok includes generic_pbs_ok, which refuses a (k, N, level) without a general key format: past this
  // point vp_layout can fail for sizes only
  if (!vp_params_ok(k, N, level, base_log)) {
    set_error("vertical_packing: unsupported parameters k=%u N=%u level=%u base_log=%u", k, N, level, base_log);
    return -2;
  }
  const VpLayout lay = vp_layout(k, N, level, r, m, tau, lookups);
  if (!lay.ok) {
    set_error("vertical_packing: r=%u mbr_size=%u tau=%u num_lookups=%u overflow the call's sizes", r, m, tau, lookups);
    return -3;
  }
  if (const int rc = scratch_refused("vertical_packing", scratch, scratch_bytes, lay.bytes)) return rc;

  CHIP_CHECK(hipSetDevice((int)gpu_index));
  hipStream_t s = (hipStream_t)stream;
  const CallScratch own(scratch, lay.bytes, s);
  char* base = own.base;

  // ---- the GGSWs: conversion and the per-key gate (the call's one host synchronisation) ----
  void* keys = base + lay.keys;
  if (r + m > 0) {
    double maxG;
    const KeyFormat f = generic_key_format(k, N, level);
    unsigned long long* sink = key_spectrum_sink(s);
    int rc = vp_convert_launch(s, keys, ggsw_in, (uint64_t)lookups * (r + m), k, N, level, sink);
    const int rs = key_spectrum_record(s, rc == 0 ? keys : nullptr, f, 0, k, N, level, sink);
    if (rc == 0) rc = rs;
    // the measured value reaches the caller on a gate refusal too: it is what explains the refusal
    maxG = concrete_hip_key_spectrum_max(keys);
    if (ggsw_spectrum_max && maxG >= 0.0) *ggsw_spectrum_max = maxG;
    if (rc == 0) rc = key_bound_check(keys, KeyKind::GENERIC, k, N, level, base_log);
    key_spectrum_forget(keys);  // the record was this call's: the scratch address will hold other keys
    if (rc != 0) return rc;
  } else if (ggsw_spectrum_max) {
    *ggsw_spectrum_max = 0.0;
  }

  // ---- tree ----
  const uint64_t G = (uint64_t)(k + 1) * N;
  const uint32_t outs = lookups * tau;
  uint64_t* cur = (uint64_t*)(base + lay.a);
  uint64_t* other = (uint64_t*)(base + lay.b);
  int rc = 0;
  if (r == 0) {
    const uint64_t total = (uint64_t)outs * G;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 256ull * 64);
    hipLaunchKernelGGL(vp_seed_kernel, dim3(blocks), dim3(256), 0, s, cur, glwe_in, lut_vector, G, (uint64_t)k * N,
                       (uint64_t)tau, total);
  }
  CmuxArgs c{s, nullptr, nullptr, keys, k, N, level, base_log, 0, 0, r + m, 0, 0, (unsigned long long*)resid_bits};
  for (uint32_t j = 0; j < r && rc == 0; ++j) {
    c.per_lookup = tau << (r - 1 - j);
    c.count = lookups * c.per_lookup;
    c.key_index = r - 1 - j;
    if (j == 0) {
      c.dst = cur, c.src = lut_vector;
      rc = vp_cmux_launch(CmuxMode::LEAF, c);
    } else {
      c.dst = other, c.src = cur;
      rc = vp_cmux_launch(CmuxMode::PAIR, c);
      std::swap(cur, other);
    }
  }
  if (rc == 0 && glwe_tree_out)
    CHIP_CHECK(hipMemcpyAsync(glwe_tree_out, cur, (uint64_t)outs * G * 8, hipMemcpyDeviceToDevice, s));

  // ---- rotation and extraction ----
  c.per_lookup = tau, c.count = outs;
  for (uint32_t j = m; j-- > 0 && rc == 0;) {
    c.dst = other, c.src = cur;
    c.key_index = r + j;
    c.rot = 1u << (m - 1 - j);
    rc = vp_cmux_launch(CmuxMode::ROTATE, c);
    std::swap(cur, other);
  }
  if (rc == 0 && lwe_array_out) rc = vp_extract_launch(s, lwe_array_out, cur, outs, k, N);
  return rc;
}

static ScratchRegistry g_vp_scratch;  // the buffers handed out by the two scratch calls

static void vp_scratch(const char* what, void* stream, uint32_t gpu_index, int8_t** buffer, uint32_t k, uint32_t N,
                       uint32_t level, uint32_t r, uint32_t m, uint32_t tau, bool allocate) {
  if (!buffer) {
    set_error("null buffer pointer");
    die(what);
  }
  *buffer = nullptr;
  const uint64_t bytes = concrete_hip_vertical_packing_scratch_bytes(k, N, level, r, m, tau, 1);
  if (bytes == 0) {
    set_error("scratch: unsupported parameters k=%u N=%u level=%u r=%u mbr_size=%u tau=%u", k, N, level, r, m, tau);
    die(what);
  }
  if (allocate) *buffer = g_vp_scratch.allocate(gpu_index, bytes, stream);  // else NULL: the call takes pool scratch
}

static uint64_t vp_scratch_size(const char* what, const int8_t* buffer) {
  return g_vp_scratch.size_of(what, "this call's scratch function", buffer);
}

}  // namespace chip

using namespace chip;

extern "C" {

int concrete_hip_vertical_packing_supported(uint32_t glwe_dimension, uint32_t polynomial_size, uint32_t level_count,
                                            uint32_t base_log) {
  return vp_params_ok(glwe_dimension, polynomial_size, level_count, base_log) ? 1 : 0;
}

uint64_t concrete_hip_vertical_packing_scratch_bytes(uint32_t glwe_dimension, uint32_t polynomial_size,
                                                     uint32_t level_count, uint32_t r, uint32_t mbr_size, uint32_t tau,
                                                     uint32_t num_lookups) {
  if (polynomial_size == 0 || mbr_size > log2u(polynomial_size)) return 0;
  const VpLayout l = vp_layout(glwe_dimension, polynomial_size, level_count, r, mbr_size, tau, num_lookups);
  return l.ok ? l.bytes : 0;
}

int concrete_hip_vertical_packing(void* stream, uint32_t gpu_index, uint64_t* lwe_array_out, uint64_t* glwe_tree_out,
                                  const uint64_t* ggsw_in, const uint64_t* lut_vector, uint32_t glwe_dimension,
                                  uint32_t polynomial_size, uint32_t base_log, uint32_t level_count, uint32_t r,
                                  uint32_t mbr_size, uint32_t tau, uint32_t num_lookups, void* scratch,
                                  uint64_t scratch_bytes, uint64_t* resid_bits, double* ggsw_spectrum_max) {
  return vp_run(stream, gpu_index, lwe_array_out, glwe_tree_out, ggsw_in, lut_vector, nullptr, glwe_dimension,
                polynomial_size, base_log, level_count, r, mbr_size, tau, num_lookups, scratch, scratch_bytes,
                resid_bits, ggsw_spectrum_max);
}

void scratch_cuda_cmux_tree_64(void* stream, uint32_t gpu_index, int8_t** cmux_tree_buffer, uint32_t glwe_dimension,
                               uint32_t polynomial_size, uint32_t level_count, uint32_t r, uint32_t tau,
                               uint32_t max_shared_memory, bool allocate_gpu_memory) {
  (void)max_shared_memory;
  vp_scratch("scratch_cuda_cmux_tree_64", stream, gpu_index, cmux_tree_buffer, glwe_dimension, polynomial_size,
             level_count, r, 0, tau, allocate_gpu_memory);
}

void cuda_cmux_tree_64(void* stream, uint32_t gpu_index, void* glwe_array_out, const void* ggsw_in,
                       const void* lut_vector, int8_t* cmux_tree_buffer, uint32_t glwe_dimension,
                       uint32_t polynomial_size, uint32_t base_log, uint32_t level_count, uint32_t r, uint32_t tau,
                       uint32_t max_shared_memory) {
  (void)max_shared_memory;
  const uint64_t bytes = vp_scratch_size("cuda_cmux_tree_64", cmux_tree_buffer);
  if (!glwe_array_out) {
    set_error("null output");
    die("cuda_cmux_tree_64");
  }
  if (vp_run(stream, gpu_index, nullptr, (uint64_t*)glwe_array_out, (const uint64_t*)ggsw_in,
             (const uint64_t*)lut_vector, nullptr, glwe_dimension, polynomial_size, base_log, level_count, r, 0, tau, 1,
             cmux_tree_buffer, bytes, nullptr, nullptr) != 0)
    die("cuda_cmux_tree_64");
}

void cleanup_cuda_cmux_tree(void* stream, uint32_t gpu_index, int8_t** cmux_tree_buffer) {
  g_vp_scratch.release(gpu_index, cmux_tree_buffer, stream);
}

void scratch_cuda_blind_rotation_sample_extraction_64(void* stream, uint32_t gpu_index, int8_t** br_se_buffer,
                                                      uint32_t glwe_dimension, uint32_t polynomial_size,
                                                      uint32_t level_count, uint32_t mbr_size, uint32_t tau,
                                                      uint32_t max_shared_memory, bool allocate_gpu_memory) {
  (void)max_shared_memory;
  vp_scratch("scratch_cuda_blind_rotation_sample_extraction_64", stream, gpu_index, br_se_buffer, glwe_dimension,
             polynomial_size, level_count, 0, mbr_size, tau, allocate_gpu_memory);
}

void cuda_blind_rotate_and_sample_extraction_64(void* stream, uint32_t gpu_index, void* lwe_out, const void* ggsw_in,
                                                const void* lut_vector, int8_t* br_se_buffer, uint32_t mbr_size,
                                                uint32_t tau, uint32_t glwe_dimension, uint32_t polynomial_size,
                                                uint32_t base_log, uint32_t level_count, uint32_t max_shared_memory) {
  (void)max_shared_memory;
  const char* what = "cuda_blind_rotate_and_sample_extraction_64";
  const uint64_t bytes = vp_scratch_size(what, br_se_buffer);
  if (!lwe_out || !lut_vector) {
    set_error("null pointer");
    die(what);
  }
  if (vp_run(stream, gpu_index, (uint64_t*)lwe_out, nullptr, (const uint64_t*)ggsw_in, nullptr,
             (const uint64_t*)lut_vector, glwe_dimension, polynomial_size, base_log, level_count, 0, mbr_size, tau, 1,
             br_se_buffer, bytes, nullptr, nullptr) != 0)
    die(what);
}

void cleanup_cuda_blind_rotation_sample_extraction(void* stream, uint32_t gpu_index, int8_t** br_se_buffer) {
  g_vp_scratch.release(gpu_index, br_se_buffer, stream);
}

}  // extern "C"
